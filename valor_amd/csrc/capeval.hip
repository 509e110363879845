// Caption evaluation on the device: corpus BLEU-1..4, ROUGE-L and CIDEr of one hypothesis row per clip (valor_amd/capeval.py states the
// rules; cococaption/pycocoevalcap bleu/bleu_scorer.py:201-266 'closest', rouge/rouge.py:47-77, cider/cider_scorer.py:96-195).
// See include/valor_hip.h for the contract and the table format (valor_capeval_tables, built by capeval.capeval_tables).
//
// The n-gram, tf-idf and BLEU passes are those of reward.hip (same keys: (t_i + 1) in 16-bit field i of one 64-bit integer, 65535 = a symbol
// outside the vocabulary); its few helpers are duplicated here so that reward.hip stays as it is. New: the four BLEU orders and their
// integers, ROUGE-L, and a second launch that reduces the rows to the corpus values.
//
// Tiling: ONE workgroup of four waves per hypothesis row. LDS (39 KB: four workgroups per CU) = reward.hip's arrays plus
//   mask [128][2] uint64  the match mask of the distinct symbol that first occurs at position i: bit j = (tok[j] == tok[i])
//   hkey / hidx [256]     an open-addressing table symbol + 1 -> that position (at most 128 entries: it never fills)
// ROUGE-L is a longest common subsequence per (hypothesis, reference) pair, done bit-parallel: the hypothesis (<= 128 symbols) is two
// 64-bit words, V starts as all ones, and a reference symbol with match mask M updates V = (V + (V & M)) | (V & ~M), the carry of the
// low word entering the high one; LCS = the zero bits of V (bits at and above the hypothesis length stay 1). ONE LANE per reference walks
// its symbols (any number of them), a clip with more than 256 references loops; the maxima of lcs and lcs / len(ref) are exact (integer,
// and a maximum of correctly rounded quotients), so their reduction order does not matter.
// Arithmetic: fp64 everywhere, fixed reduction orders (shuffle trees, LDS slots summed by one thread); integer atomics only (LDS min / CAS /
// add); idf and reference tf-idf are the host's bits. Two launches on the same input give the same bits.
#include "common.h"
#include "../../include/valor_hip.h"
#include <math.h>

#define CE_THREADS 256
#define CE_WAVES 4
#define CE_MAXL 128
#define CE_SLOTS (4 * CE_MAXL)
#define CE_STAGE 1536
#define CE_UNKNOWN 65535ull
#define CE_HASH 256

typedef valor_capeval_tables CapevalTables;          // the one definition: include/valor_hip.h
typedef valor_capeval_summary CapevalSummary;

// index of `k` in the sorted keys[lo, hi), -1 if absent
DEVINL int ce_find(const uint64_t* keys, int lo, int hi, uint64_t k) {
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && keys[lo] == k) ? lo : -1;
}
DEVINL double ce_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
DEVINL int ce_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
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

// (prod_{j <= k} (correct_j + 1e-15) / (guess_j + 1e-9))^(1 / k), k = 1..4, with the brevity penalty (bleu_scorer.py:234-242, 251-259)
template <typename I>
DEVINL void ce_bleu(const I* correct, const I* guess, I testlen, I reflen, double* out) {
    double b = 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b *= ((double)correct[k] + 1e-15) / ((double)guess[k] + 1e-9);
        out[k] = pow(b, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)testlen + 1e-15) / ((double)reflen + 1e-9);
    if (ratio < 1.0) {
        const double bp = exp(1.0 - 1.0 / ratio);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] *= bp;
    }
}

__global__ __launch_bounds__(CE_THREADS) void caption_metrics_kernel(const int64_t* __restrict__ seq, int64_t ld, int L, int64_t eos, int vocab,
                                                                     const int32_t* __restrict__ clip_idx, CapevalTables T,
                                                                     double* __restrict__ cider, double* __restrict__ rouge,
                                                                     double* __restrict__ bleu, int32_t* __restrict__ counts) {
    __shared__ int64_t sh_tok[CE_MAXL];
    __shared__ uint64_t sh_key[CE_SLOTS];
    __shared__ double sh_x[CE_SLOTS];
    __shared__ int sh_tf[CE_SLOTS];
    __shared__ uint64_t sh_rkey[CE_STAGE];
    __shared__ double sh_rval[CE_STAGE];
    __shared__ uint64_t sh_mask[CE_MAXL][2];
    __shared__ int sh_hkey[CE_HASH], sh_hidx[CE_HASH];
    __shared__ double sh_sq[CE_WAVES][2], sh_norm[4], sh_score[CE_WAVES][4], sh_rec[CE_WAVES];
    __shared__ int sh_cut[CE_WAVES], sh_correct[CE_WAVES][2], sh_lcs[CE_WAVES];
    __shared__ unsigned long long sh_closest;

    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const int c = clip_idx[r];
    int ref0 = 0, ref1 = 0;
    if (c >= 0 && c < T.n_clips) { ref0 = T.clip_ref_ptr[c]; ref1 = T.clip_ref_ptr[c + 1]; }
    if (ref1 <= ref0) {                                    // no such clip, or a clip without references: no score (block-uniform)
        if (tid == 0) { cider[r] = nanv; rouge[r] = nanv; }
        if (tid < 4) bleu[(int64_t)r * 4 + tid] = nanv;
        if (tid < 10) counts[(int64_t)r * 10 + tid] = -1;
        return;
    }

    // ---- pass 1: symbols, the cut, the keys
    int64_t t = eos;
    if (tid < L) t = seq[(int64_t)r * ld + tid];
    if (tid < CE_MAXL) sh_tok[tid] = t;
    sh_hkey[tid] = 0;                                      // CE_HASH == CE_THREADS
    {
        const unsigned long long hit = __ballot(tid < L && t == eos);
        if (lane == 0) sh_cut[wave] = hit ? wave * 64 + __builtin_ctzll(hit) : L;
        if (tid == 0) sh_closest = ~0ull;
    }
    const int k0 = T.ref_key_ptr[ref0], k1 = T.ref_key_ptr[ref1];
    const bool staged = k1 - k0 <= CE_STAGE;
    if (staged)
        for (int i = tid; i < k1 - k0; i += CE_THREADS) { sh_rkey[i] = T.ref_keys[k0 + i]; sh_rval[i] = T.ref_vals[k0 + i]; }
    __syncthreads();
    int len = sh_cut[0];
#pragma unroll
    for (int w = 1; w < CE_WAVES; ++w) len = sh_cut[w] < len ? sh_cut[w] : len;
    len = len < L ? len : L;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * CE_THREADS, n = s >> 7, i = s & (CE_MAXL - 1);          // the (n + 1)-gram starting at i
        uint64_t key = 0;
        if (i + n < len) {
            for (int j = 0; j <= n; ++j) {
                const int64_t w = sh_tok[i + j];
                const uint64_t code = (w >= 0 && w < (int64_t)vocab) ? (uint64_t)w + 1 : CE_UNKNOWN;
                key |= code << (16 * j);
            }
        }
        sh_key[s] = key;
    }
    __syncthreads();

    // ---- pass 2: counts. tf on the first occurrence of an n-gram, 0 on its repeats
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * CE_THREADS, n = s >> 7, i = s & (CE_MAXL - 1);
        const uint64_t key = sh_key[s];
        int cnt = 0;
        bool first = true;
        if (key) {
            const bool unk = ((key & 0xffff) == CE_UNKNOWN) || (((key >> 16) & 0xffff) == CE_UNKNOWN) || (((key >> 32) & 0xffff) == CE_UNKNOWN) ||
                             ((key >> 48) == CE_UNKNOWN);
            const int starts = len - n;
            for (int j = 0; j < starts; ++j) {
                bool eq = sh_key[(n << 7) + j] == key;
                if (eq && unk)
                    for (int q = 0; q <= n; ++q) eq = eq && sh_tok[i + q] == sh_tok[j + q];
                cnt += eq ? 1 : 0;
                first = first && !(eq && j < i);
            }
        }
        sh_tf[s] = (key && first) ? cnt : 0;
    }
    __syncthreads();

    // ---- pass 3: hypothesis tf-idf and norms; BLEU clipped counts; the closest reference length; the match masks of the LCS
    const int b0 = T.clip_bleu_ptr[c], b1 = T.clip_bleu_ptr[c + 1];
    double sq[2];
    int corr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * CE_THREADS;
        const int tf = sh_tf[s];
        double x = 0.0;
        int cc = 0;
        if (tf) {
            const uint64_t key = sh_key[s];
            const int g = T.n_global > 0 ? ce_find(T.g_keys, 0, T.n_global, key) : -1;
            x = (double)tf * (g >= 0 ? T.g_idf[g] : T.ref_len);
            const int m = ce_find(T.bleu_keys, b0, b1, key);
            if (m >= 0) { const int mc = T.bleu_cnt[m]; cc = mc < tf ? mc : tf; }
        }
        sh_x[s] = x;
        sq[h] = ce_wave_sum(x * x);
        corr[h] = ce_wave_sum_i(cc);
    }
    if (lane == 0) { sh_sq[wave][0] = sq[0]; sh_sq[wave][1] = sq[1]; sh_correct[wave][0] = corr[0]; sh_correct[wave][1] = corr[1]; }
    for (int q = ref0 + tid; q < ref1; q += CE_THREADS) {
        const int l = T.ref_tokens[q];
        const unsigned d = (unsigned)(l > len ? l - len : len - l);
        atomicMin(&sh_closest, ((unsigned long long)d << 32) | (unsigned)l);          // integer: (distance, length), ties to the shorter
    }
    if (tid < CE_MAXL && sh_tf[tid]) {                     // slot (n = 1, i = tid): a distinct symbol at its first position
        const int64_t w = sh_tok[tid];
        if (w >= 0 && w < (int64_t)vocab) {                // a symbol outside the vocabulary is in no reference
            uint64_t m0 = 0, m1 = 0;
            for (int j = tid; j < len; ++j)
                if (sh_tok[j] == w) { if (j < 64) m0 |= 1ull << j; else m1 |= 1ull << (j - 64); }
            sh_mask[tid][0] = m0;
            sh_mask[tid][1] = m1;
            const int code = (int)w + 1;
            unsigned hs = ce_hash((int)w);
            while (atomicCAS(&sh_hkey[hs], 0, code) != 0) hs = (hs + 1) & (CE_HASH - 1);          // one inserter per symbol, <= 128 of 256 slots
            sh_hidx[hs] = tid;
        }
    }
    __syncthreads();
    // slots 0..127 (n = 1) belong to waves 0, 1 at h = 0; 128..255 (n = 2) to waves 2, 3 at h = 0; n = 3, 4 the same at h = 1
    if (tid < 4) sh_norm[tid] = sqrt(sh_sq[(tid & 1) * 2][tid >> 1] + sh_sq[(tid & 1) * 2 + 1][tid >> 1]);

    // ---- pass 4: ROUGE-L. One lane per reference, bit-parallel LCS against the hypothesis' two words
    {
        int best = 0;
        double rec = 0.0;
        for (int q = ref0 + tid; q < ref1; q += CE_THREADS) {
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

    // ---- pass 5: CIDEr against every reference of the clip
    const uint64_t* rkeys = staged ? sh_rkey : T.ref_keys + k0;
    const double* rvals = staged ? sh_rval : T.ref_vals + k0;
    const int lh = len > 1 ? len - 1 : 0;                  // the hypothesis' bigram count: the reference's "length"
    double score[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = ref0 + wave; q < ref1; q += CE_WAVES) {
        const int lo = T.ref_key_ptr[q] - k0, hi = T.ref_key_ptr[q + 1] - k0;
        double val[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = lane + 64 * k;
            if (sh_tf[s]) {
                const int m = ce_find(rkeys, lo, hi, sh_key[s]);
                if (m >= 0) {
                    const double x = sh_x[s], y = rvals[m];
                    val[k >> 1] += (x < y ? x : y) * y;
                }
            }
        }
        const double delta = (double)(lh - T.ref_bigrams[q]);
        const double pen = exp(-(delta * delta) / (2.0 * 6.0 * 6.0));
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double v = ce_wave_sum(val[n]);
            const double nh = sh_norm[n], nr = T.ref_norm[(int64_t)q * 4 + n];
            if (nh != 0.0 && nr != 0.0) v /= nh * nr;
            score[n] += v * pen;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) sh_score[wave][n] = score[n];
    }
    __syncthreads();

    // ---- pass 6: combine
    if (tid == 0) {
        double sum = 0.0;
#pragma unroll
        for (int n = 0; n < 4; ++n) sum += (sh_score[0][n] + sh_score[1][n]) + (sh_score[2][n] + sh_score[3][n]);
        cider[r] = sum / 4.0 / (double)(ref1 - ref0) * 10.0;
        int lcs = sh_lcs[0];
        double rec = sh_rec[0];
#pragma unroll
        for (int w = 1; w < CE_WAVES; ++w) { lcs = sh_lcs[w] > lcs ? sh_lcs[w] : lcs; rec = fmax(rec, sh_rec[w]); }
        const double prec = len > 0 ? (double)lcs / (double)len : 0.0;
        const double beta2 = 1.2 * 1.2;
        rouge[r] = (prec != 0.0 && rec != 0.0) ? ((1.0 + beta2) * prec * rec) / (rec + beta2 * prec) : 0.0;
        const int correct[4] = {sh_correct[0][0] + sh_correct[1][0], sh_correct[2][0] + sh_correct[3][0], sh_correct[0][1] + sh_correct[1][1],
                                sh_correct[2][1] + sh_correct[3][1]};
        int guess[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) guess[k] = len - k > 0 ? len - k : 0;
        const int reflen = (int)(unsigned)(sh_closest & 0xffffffffull);
        double b[4];
        ce_bleu<int>(correct, guess, len, reflen, b);
        int32_t* cnt = counts + (int64_t)r * 10;
#pragma unroll
        for (int k = 0; k < 4; ++k) { bleu[(int64_t)r * 4 + k] = b[k]; cnt[k] = correct[k]; cnt[4 + k] = guess[k]; }
        cnt[8] = len;
        cnt[9] = reflen;
    }
}

// The corpus reduction: one workgroup. Thread t sums the rows t, t + 256, .. in order, then a shuffle tree per wave and the four waves in
// order: a fixed order for the two fp64 sums. The integer totals go through LDS integer adds.
__global__ __launch_bounds__(CE_THREADS) void caption_metrics_reduce_kernel(const double* __restrict__ cider, const double* __restrict__ rouge,
                                                                            const int32_t* __restrict__ counts, int R,
                                                                            CapevalSummary* __restrict__ summary) {
    __shared__ double sh_f[CE_WAVES][2];
    __shared__ unsigned long long sh_i[11];                // the ten totals and the number of rows without a score
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 11) sh_i[tid] = 0ull;
    __syncthreads();
    double sc = 0.0, sr = 0.0;
    long long tot[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long bad = 0;
    for (int r = tid; r < R; r += CE_THREADS) {
        const int32_t* cnt = counts + (int64_t)r * 10;
        sc += cider[r];
        sr += rouge[r];
        if (cnt[8] < 0) { ++bad; continue; }
#pragma unroll
        for (int k = 0; k < 10; ++k) tot[k] += cnt[k];
    }
    sc = ce_wave_sum(sc);
    sr = ce_wave_sum(sr);
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
        ce_bleu<long long>(total, total + 4, total[8], total[9], b);
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
    if (R < 0 || L < 1 || L > CE_MAXL || vocab < 1 || vocab > 65534 || eos < 0 || eos >= vocab || ld < L) return VALOR_ERR_ARG;
    if (R == 0) {
        if (summary && hipMemsetAsync(summary, 0, sizeof(CapevalSummary), (hipStream_t)stream) != hipSuccess) return VALOR_ERR_LAUNCH;
        return VALOR_OK;
    }
    if (!seq || !clip_idx || !tables || !cider || !rouge || !bleu || !counts || !summary) return VALOR_ERR_ARG;
    const CapevalTables& t = *tables;
    if (!t.clip_ref_ptr || !t.ref_key_ptr || !t.ref_keys || !t.ref_vals || !t.ref_norm || !t.ref_bigrams || !t.ref_tokens || !t.clip_bleu_ptr ||
        !t.bleu_keys || !t.bleu_cnt || !t.ref_sym_ptr || !t.ref_syms)
        return VALOR_ERR_ARG;
    if (t.n_clips < 1 || t.n_global < 0 || (t.n_global > 0 && (!t.g_keys || !t.g_idf))) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(caption_metrics_kernel, dim3(R), dim3(CE_THREADS), 0, (hipStream_t)stream, seq, ld, L, eos, vocab, clip_idx, t, cider, rouge,
                       bleu, counts);
    hipLaunchKernelGGL(caption_metrics_reduce_kernel, dim3(1), dim3(CE_THREADS), 0, (hipStream_t)stream, cider, rouge, counts, R, summary);
    return valor_launch_status();
}
