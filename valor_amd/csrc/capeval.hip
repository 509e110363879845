// Caption evaluation on the device: corpus BLEU-1..4, ROUGE-L and CIDEr of one hypothesis row per clip (valor_amd/capeval.py states the
// rules; cococaption/pycocoevalcap bleu/bleu_scorer.py:201-266 'closest', rouge/rouge.py:47-77, cider/cider_scorer.py:96-195).
// See include/valor_hip.h for the contract and the table format (valor_capeval_tables, built by capeval.capeval_tables).
//
// The n-gram, tf-idf, CIDEr and BLEU passes are the core of ngram.h (keys, tiling, passes and arithmetic are described there), shared with
// reward.hip. Here: the four BLEU orders and their integers, ROUGE-L, and a second launch that reduces the rows to the corpus values.
//
// Tiling: ONE workgroup of four waves per hypothesis row. LDS (39 KB: four workgroups per CU) = the core's NgramLds plus
//   mask [128][2] uint64  the match mask of the distinct symbol that first occurs at position i: bit j = (tok[j] == tok[i])
//   hkey / hidx [256]     an open-addressing table symbol + 1 -> that position (at most 128 entries: it never fills)
// ROUGE-L is a longest common subsequence per (hypothesis, reference) pair, done bit-parallel: the hypothesis (<= 128 symbols) is two
// 64-bit words, V starts as all ones, and a reference symbol with match mask M updates V = (V + (V & M)) | (V & ~M), the carry of the
// low word entering the high one; LCS = the zero bits of V (bits at and above the hypothesis length stay 1). ONE LANE per reference walks
// its symbols (any number of them), a clip with more than 256 references loops; the maxima of lcs and lcs / len(ref) are exact (integer,
// and a maximum of correctly rounded quotients), so their reduction order does not matter.
#include "common.h"
#include "../../include/valor_hip.h"
#include "ngram.h"

#define CE_HASH 256

typedef valor_capeval_tables CapevalTables;          // the one definition: include/valor_hip.h
typedef valor_capeval_summary CapevalSummary;

DEVINL double ce_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
DEVINL int ce_wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    return v;
}
DEVINL unsigned ce_hash(int sym) { return ((unsigned)sym * 2654435761u) >> 24; }          // 8 bits: CE_HASH slots

__global__ __launch_bounds__(NG_THREADS) void caption_metrics_kernel(const int64_t* __restrict__ seq, int64_t ld, int L, int64_t eos, int vocab,
                                                                     const int32_t* __restrict__ clip_idx, CapevalTables T,
                                                                     double* __restrict__ cider, double* __restrict__ rouge,
                                                                     double* __restrict__ bleu, int32_t* __restrict__ counts) {
    __shared__ NgramLds S;
    __shared__ uint64_t sh_mask[NG_MAXL][2];
    __shared__ int sh_hkey[CE_HASH], sh_hidx[CE_HASH];
    __shared__ double sh_rec[NG_WAVES];
    __shared__ int sh_lcs[NG_WAVES];

    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = clip_idx[r];
    int ref0, ref1;
    ng_clip_refs(T, c, ref0, ref1);
    if (ref1 <= ref0) {                                    // no such clip, or a clip without references: no score (block-uniform)
        const double nanv = __longlong_as_double(0x7ff8000000000000ll);
        if (tid == 0) { cider[r] = nanv; rouge[r] = nanv; }
        if (tid < 4) bleu[(int64_t)r * 4 + tid] = nanv;
        if (tid < 10) counts[(int64_t)r * 10 + tid] = -1;
        return;
    }
    sh_hkey[tid] = 0;                                      // CE_HASH == NG_THREADS; ng_load_row's first barrier covers it
    int k0;
    bool staged;
    const int len = ng_load_row(S, T, seq, ld, L, eos, vocab, ref0, ref1, k0, staged);
    __syncthreads();

    // ---- the core's pass 3, and in it the match masks of the LCS
    ng_score_slots(S, T, c, ref0, ref1, len);
    if (tid < NG_MAXL && S.tf[tid]) {                     // slot (n = 1, i = tid): a distinct symbol at its first position
        const int64_t w = S.tok[tid];
        if (w >= 0 && w < (int64_t)vocab) {                // a symbol outside the vocabulary is in no reference
            uint64_t m0 = 0, m1 = 0;
            for (int j = tid; j < len; ++j)
                if (S.tok[j] == w) { if (j < 64) m0 |= 1ull << j; else m1 |= 1ull << (j - 64); }
            sh_mask[tid][0] = m0;
            sh_mask[tid][1] = m1;
            const int code = (int)w + 1;
            unsigned hs = ce_hash((int)w);
            while (atomicCAS(&sh_hkey[hs], 0, code) != 0) hs = (hs + 1) & (CE_HASH - 1);          // one inserter per symbol, <= 128 of 256 slots
            sh_hidx[hs] = tid;
        }
    }
    __syncthreads();
    ng_norms(S);

    // ---- ROUGE-L. One lane per reference, bit-parallel LCS against the hypothesis' two words
    {
        int best = 0;
        double rec = 0.0;
        for (int q = ref0 + tid; q < ref1; q += NG_THREADS) {
            const int s0 = T.ref_sym_ptr[q], s1 = T.ref_sym_ptr[q + 1];
            uint64_t v0 = ~0ull, v1 = ~0ull;
            for (int p = s0; p < s1; ++p) {
                const int sym = (int)T.ref_syms[p], code = sym + 1;
                uint64_t m0 = 0, m1 = 0;
                unsigned hs = ce_hash(sym);
                for (int probe = 0; probe < CE_HASH; ++probe) {
                    const int k = sh_hkey[hs];
                    if (k == 0) break;
                    if (k == code) { const int i = sh_hidx[hs]; m0 = sh_mask[i][0]; m1 = sh_mask[i][1]; break; }
                    hs = (hs + 1) & (CE_HASH - 1);
                }
                const uint64_t u0 = v0 & m0, u1 = v1 & m1;
                const uint64_t lo = v0 + u0;
                const uint64_t hi = v1 + u1 + (lo < v0 ? 1ull : 0ull);
                v0 = lo | (v0 & ~m0);
                v1 = hi | (v1 & ~m1);
            }
            const int lcs = __popcll(~v0) + __popcll(~v1);
            best = lcs > best ? lcs : best;
            if (s1 > s0) rec = fmax(rec, (double)lcs / (double)(s1 - s0));
        }
        best = ce_wave_max_i(best);
        rec = ce_wave_max(rec);
        if (lane == 0) { sh_lcs[wave] = best; sh_rec[wave] = rec; }
    }
    __syncthreads();
    ng_cider(S, T, ref0, ref1, k0, staged, len);
    __syncthreads();

    // ---- combine
    if (tid == 0) {
        cider[r] = ng_cider_total(S, ref0, ref1);
        int lcs = sh_lcs[0];
        double rec = sh_rec[0];
#pragma unroll
        for (int w = 1; w < NG_WAVES; ++w) { lcs = sh_lcs[w] > lcs ? sh_lcs[w] : lcs; rec = fmax(rec, sh_rec[w]); }
        const double prec = len > 0 ? (double)lcs / (double)len : 0.0;
        const double beta2 = 1.2 * 1.2;
        rouge[r] = (prec != 0.0 && rec != 0.0) ? ((1.0 + beta2) * prec * rec) / (rec + beta2 * prec) : 0.0;
        int correct[4], guess[4];
        const int reflen = ng_correct(S, len, correct, guess);
        double b[4];
        ng_bleu<int>(correct, guess, len, reflen, b);
        int32_t* cnt = counts + (int64_t)r * 10;
#pragma unroll
        for (int k = 0; k < 4; ++k) { bleu[(int64_t)r * 4 + k] = b[k]; cnt[k] = correct[k]; cnt[4 + k] = guess[k]; }
        cnt[8] = len;
        cnt[9] = reflen;
    }
}

// The corpus reduction: one workgroup. Thread t sums the rows t, t + 256, .. in order, then a shuffle tree per wave and the four waves in
// order: a fixed order for the two fp64 sums. The integer totals go through LDS integer adds.
__global__ __launch_bounds__(NG_THREADS) void caption_metrics_reduce_kernel(const double* __restrict__ cider, const double* __restrict__ rouge,
                                                                            const int32_t* __restrict__ counts, int R,
                                                                            CapevalSummary* __restrict__ summary) {
    __shared__ double sh_f[NG_WAVES][2];
    __shared__ unsigned long long sh_i[11];                // the ten totals and the number of rows without a score
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 11) sh_i[tid] = 0ull;
    __syncthreads();
    double sc = 0.0, sr = 0.0;
    long long tot[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long bad = 0;
    for (int r = tid; r < R; r += NG_THREADS) {
        const int32_t* cnt = counts + (int64_t)r * 10;
        sc += cider[r];
        sr += rouge[r];
        if (cnt[8] < 0) { ++bad; continue; }
#pragma unroll
        for (int k = 0; k < 10; ++k) tot[k] += cnt[k];
    }
    sc = ng_wave_sum(sc);
    sr = ng_wave_sum(sr);
    if (lane == 0) { sh_f[wave][0] = sc; sh_f[wave][1] = sr; }
#pragma unroll
    for (int k = 0; k < 10; ++k)
        if (tot[k]) atomicAdd(&sh_i[k], (unsigned long long)tot[k]);
    if (bad) atomicAdd(&sh_i[10], (unsigned long long)bad);
    __syncthreads();
    if (tid == 0) {
        long long total[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) { total[k] = (long long)sh_i[k]; summary->total[k] = total[k]; }
        double b[4];
        ng_bleu<long long>(total, total + 4, total[8], total[9], b);
        const double rl = ((sh_f[0][1] + sh_f[1][1]) + (sh_f[2][1] + sh_f[3][1])) / (double)R;
        const double cd = ((sh_f[0][0] + sh_f[1][0]) + (sh_f[2][0] + sh_f[3][0])) / (double)R;
        const bool ok = sh_i[10] == 0ull;
        const double nanv = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
        for (int k = 0; k < 4; ++k) summary->value[k] = ok ? b[k] : nanv;
        summary->value[4] = ok ? rl : nanv;
        summary->value[5] = ok ? cd : nanv;
    }
}

extern "C" int valor_caption_metrics(void* stream, const int64_t* seq, int64_t ld, int R, int L, int64_t eos, int vocab, const int32_t* clip_idx,
                                     const CapevalTables* tables, double* cider, double* rouge, double* bleu, int32_t* counts,
                                     CapevalSummary* summary) {
    if (ng_check_args(seq, ld, R, L, eos, vocab, clip_idx, tables) != VALOR_OK) return VALOR_ERR_ARG;
    if (R == 0) {
        if (summary && hipMemsetAsync(summary, 0, sizeof(CapevalSummary), (hipStream_t)stream) != hipSuccess) return VALOR_ERR_LAUNCH;
        return VALOR_OK;
    }
    if (!cider || !rouge || !bleu || !counts || !summary || !tables->ref_sym_ptr || !tables->ref_syms) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(caption_metrics_kernel, dim3(R), dim3(NG_THREADS), 0, (hipStream_t)stream, seq, ld, L, eos, vocab, clip_idx, *tables, cider, rouge,
                       bleu, counts);
    hipLaunchKernelGGL(caption_metrics_reduce_kernel, dim3(1), dim3(NG_THREADS), 0, (hipStream_t)stream, cider, rouge, counts, R, summary);
    return valor_launch_status();
}
