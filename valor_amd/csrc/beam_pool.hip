// One step of the beam search with a pool of finished hypotheses (valor_beam_pool_step; the law: include/valor_hip.h, restated on the
// host by valor_amd.decode.beam_pool_step_host). The reference's search (valor_beam_select + ~10 torch launches of bookkeeping per
// step) keeps a hypothesis that produced [SEP] in the beam, where its V tied copies take the remaining slots; here it leaves for a
// pool of at most K finished hypotheses ranked by logP * inv_len[length], the beam stays K OPEN hypotheses wide, and a sample is done
// once no open hypothesis can still enter the pool. One launch per decoding step, outside the captured step, every parameter by value.
//   One 1024-thread workgroup per sample, as beam_select_kernel (misc.hip): the sample's cur rows are read once, four loads in flight;
//   every thread keeps the best KMAX = 2K of its stride in registers (its candidates arrive in index order, so a strict comparison
//   keeps equal values in index order; one thread's stride may hold all 2K winners, hence the full depth), then up to 2K rounds of a
//   workgroup-wide arg max over the threads' heads (beam_better: value, then index). The taken list goes to LDS; thread 0 walks it
//   (<= 16 entries against a pool of <= 8: a serial loop of a few hundred cycles) and leaves the new slots and the pool's row writes as
//   small tables in LDS; after one barrier all threads copy the history rows (the parent's row, position t replaced) and the pool rows.
//   Depth 8 serves K <= 4 (the flagship beam 3), depth 16 K <= 8; at 1024 threads a wave may hold 128 VGPRs, the lists take 2 * KMAX.
//   No atomics, nothing depends on wave scheduling (every reduction has a fixed order), global memory is written with vector stores.
#include "common.h"

#define BP_THREADS 1024
#define BP_MAXK 8
#define BP_NONE 0x7fffffff

DEVINL bool bp_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

template <int KMAX>
__global__ __launch_bounds__(BP_THREADS) void beam_pool_step_kernel(
    const float* __restrict__ logits, int64_t ld, int64_t rs_s, int64_t rs_k, const float* __restrict__ lse,
    const float* __restrict__ scores_in, const int64_t* __restrict__ hist_in, const float* __restrict__ inv_len, int b, int cur, int V,
    int K, int L, int t, int eos, float floor, int alpha_pos, int early, float* __restrict__ scores_out, int64_t* __restrict__ hist_out,
    int64_t* __restrict__ tok, int64_t* __restrict__ parent, uint8_t* __restrict__ active, int64_t* __restrict__ pool_seq,
    float* __restrict__ pool_logprob, float* __restrict__ pool_rank, int32_t* __restrict__ pool_len, int32_t* __restrict__ pool_ins,
    int32_t* __restrict__ pool_cnt, uint8_t* __restrict__ done) {
    __shared__ float wv[16];
    __shared__ int wi[16];
    __shared__ float sel_v[2 * BP_MAXK];                     // the taken candidates, in rank order
    __shared__ int sel_i[2 * BP_MAXK];
    __shared__ float slot_sc[BP_MAXK];                       // the new slots
    __shared__ int slot_par[BP_MAXK], slot_tok[BP_MAXK];
    __shared__ float p_rank[BP_MAXK];                        // the pool's rank scores / insertion numbers while thread 0 updates it
    __shared__ int p_ins[BP_MAXK];
    __shared__ int off_dst[BP_MAXK], off_par[BP_MAXK], off_tok[BP_MAXK];      // pool rows to write: entry, parent slot, last word
    __shared__ int n_off, now_done;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t sK = (int64_t)s * K;
    if (done[s]) {                                           // frozen (workgroup-uniform)
        for (int i = tid; i < K * L; i += BP_THREADS) hist_out[sK * L + i] = hist_in[sK * L + i];
        if (tid < K) {
            scores_out[sK + tid] = scores_in[sK + tid];
            tok[(int64_t)tid * b + s] = eos;
            parent[(int64_t)tid * b + s] = (int64_t)tid * b + s;
            active[(int64_t)tid * b + s] = 0;
        }
        return;
    }
    float lv[KMAX];
    int li[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { lv[j] = -INFINITY; li[j] = BP_NONE; }
    for (int k = 0; k < cur; ++k) {
        const float sl = scores_in[sK + k];
        if (!(sl > -INFINITY)) continue;                     // a dead slot supplies no candidates
        const int64_t row = (int64_t)s * rs_s + (int64_t)k * rs_k;
        const float* x = logits + row * ld;
        const float l = lse[row];
        for (int w0 = tid; w0 < V; w0 += 4 * BP_THREADS) {   // four loads in flight (the insertion below is a dependent chain)
            float xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = w0 + u * BP_THREADS < V ? x[w0 + u * BP_THREADS] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int w = w0 + u * BP_THREADS;
                const float c = sl + (xv[u] - l);
                if (w < V && xv[u] > floor && c > lv[KMAX - 1]) {       // (a floored column, -inf and NaN never pass)
                    lv[KMAX - 1] = c; li[KMAX - 1] = k * V + w;
#pragma unroll
                    for (int j = KMAX - 1; j > 0; --j)
                        if (lv[j] > lv[j - 1]) {
                            const float tv = lv[j]; lv[j] = lv[j - 1]; lv[j - 1] = tv;
                            const int ti = li[j]; li[j] = li[j - 1]; li[j - 1] = ti;
                        }
                }
            }
        }
    }
    int n_sel = 0;                                           // (the same in every thread)
    for (int r = 0; r < 2 * K; ++r) {
        float bv = lv[0];
        int bi = li[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (bp_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
        __syncthreads();
        bv = wv[0]; bi = wi[0];
#pragma unroll
        for (int j = 1; j < 16; ++j)
            if (bp_better(wv[j], wi[j], bv, bi)) { bv = wv[j]; bi = wi[j]; }
        __syncthreads();
        if (bi == BP_NONE) break;                            // nothing above -inf is left
        if (li[0] == bi) {                                   // this thread's head won: pop it
#pragma unroll
            for (int j = 0; j + 1 < KMAX; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; }
            lv[KMAX - 1] = -INFINITY; li[KMAX - 1] = BP_NONE;
        }
        if (tid == 0) { sel_v[r] = bv; sel_i[r] = bi; }
        n_sel = r + 1;
    }
    if (tid == 0) {
        int pn = pool_cnt[2 * s], pnext = pool_cnt[2 * s + 1];
        pn = pn < 0 ? 0 : (pn > K ? K : pn);
        for (int j = 0; j < pn; ++j) { p_rank[j] = pool_rank[sK + j]; p_ins[j] = pool_ins[sK + j]; }
        int filled = 0, noff = 0;
        for (int rho = 0; rho < n_sel && filled < K; ++rho) {
            const float c = sel_v[rho];
            const int k = sel_i[rho] / V, w = sel_i[rho] - k * V;
            const bool ends = w == eos;
            if (ends && rho >= K) continue;
            if (!ends) { slot_sc[filled] = c; slot_par[filled] = k; slot_tok[filled] = w; ++filled; }
            if (!ends && t < L - 1) continue;
            const int len = ends ? t + 1 : L;
            const float rank = c * inv_len[len];
            int dst = -1;
            if (pn < K) dst = pn++;
            else {
                int worst = 0;
                for (int j = 1; j < K; ++j)
                    if (p_rank[j] < p_rank[worst] || (p_rank[j] == p_rank[worst] && p_ins[j] > p_ins[worst])) worst = j;
                if (rank > p_rank[worst]) dst = worst;
            }
            if (dst >= 0) {
                p_rank[dst] = rank; p_ins[dst] = pnext;
                pool_logprob[sK + dst] = c; pool_rank[sK + dst] = rank; pool_len[sK + dst] = len; pool_ins[sK + dst] = pnext;
                ++pnext;
                off_dst[noff] = dst; off_par[noff] = k; off_tok[noff] = w; ++noff;
            }
        }
        for (int j = filled; j < K; ++j) { slot_sc[j] = -INFINITY; slot_par[j] = j; slot_tok[j] = eos; }
        bool d = true;
        if (t < L - 1) {
            d = filled == 0;
            if (!d && pn == K) {
                if (early) d = true;
                else {
                    float worst = p_rank[0];
                    for (int j = 1; j < K; ++j) worst = p_rank[j] < worst ? p_rank[j] : worst;
                    const float bound = slot_sc[0] * inv_len[alpha_pos ? L : t + 2];
                    d = worst >= bound;
                }
            }
        }
        pool_cnt[2 * s] = pn; pool_cnt[2 * s + 1] = pnext;
        done[s] = d ? 1 : 0;
        n_off = noff; now_done = d ? 1 : 0;
    }
    __syncthreads();
    if (tid < K) {
        scores_out[sK + tid] = slot_sc[tid];
        tok[(int64_t)tid * b + s] = slot_tok[tid];
        parent[(int64_t)tid * b + s] = (int64_t)slot_par[tid] * b + s;
        active[(int64_t)tid * b + s] = (!now_done && slot_sc[tid] > -INFINITY) ? 1 : 0;
    }
    for (int i = tid; i < K * L; i += BP_THREADS) {
        const int j = i / L, p = i - j * L;
        const int64_t v = p == t ? (int64_t)slot_tok[j] : hist_in[(sK + slot_par[j]) * L + p];
        hist_out[sK * L + i] = v;
    }
    const int no = n_off;
    for (int o = 0; o < no; ++o)                             // (an entry is rewritten by the same thread, in order)
        for (int p = tid; p < L; p += BP_THREADS) {
            const int64_t v = p < t ? hist_in[(sK + off_par[o]) * L + p] : (p == t ? (int64_t)off_tok[o] : (int64_t)eos);
            pool_seq[(sK + off_dst[o]) * L + p] = v;
        }
}

extern "C" int valor_beam_pool_step(void* stream, const float* logits, int64_t ld, int64_t row_stride_s, int64_t row_stride_k,
                                    const float* lse, const float* scores_in, const int64_t* hist_in, const float* inv_len, int b, int cur,
                                    int V, int beam, int max_len, int t, int64_t eos, float floor, int alpha_pos, int early_stopping, float* scores_out,
                                    int64_t* hist_out, int64_t* tok, int64_t* parent, uint8_t* active, int64_t* pool_seq,
                                    float* pool_logprob, float* pool_rank, int32_t* pool_len, int32_t* pool_ins, int32_t* pool_cnt,
                                    uint8_t* done) {
    if (b == 0) return VALOR_OK;
    if (!logits || !lse || !scores_in || !hist_in || !inv_len || !scores_out || !hist_out || !tok || !parent || !active || !pool_seq ||
        !pool_logprob || !pool_rank || !pool_len || !pool_ins || !pool_cnt || !done || hist_in == hist_out)
        return VALOR_ERR_ARG;
    if (b < 0 || beam < 1 || beam > BP_MAXK || cur < 1 || cur > beam || V < 1 || ld < V || row_stride_s < 0 || row_stride_k < 0)
        return VALOR_ERR_ARG;
    if ((int64_t)cur * V < 2 * beam || (int64_t)cur * V >= 0x7fffffff || max_len < 1 || max_len > 512 || t < 0 || t >= max_len ||
        eos < 0 || eos >= V || floor != floor)
        return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (beam <= 4)
        hipLaunchKernelGGL((beam_pool_step_kernel<8>), dim3((unsigned)b), dim3(BP_THREADS), 0, st, logits, ld, row_stride_s, row_stride_k, lse,
                           scores_in, hist_in, inv_len, b, cur, V, beam, max_len, t, (int)eos, floor, alpha_pos, early_stopping, scores_out,
                           hist_out, tok, parent, active, pool_seq, pool_logprob, pool_rank, pool_len, pool_ins, pool_cnt, done);
    else
        hipLaunchKernelGGL((beam_pool_step_kernel<16>), dim3((unsigned)b), dim3(BP_THREADS), 0, st, logits, ld, row_stride_s, row_stride_k, lse,
                           scores_in, hist_in, inv_len, b, cur, V, beam, max_len, t, (int)eos, floor, alpha_pos, early_stopping, scores_out,
                           hist_out, tok, parent, active, pool_seq, pool_logprob, pool_rank, pool_len, pool_ins, pool_cnt, done);
    return valor_launch_status();
}
