// One step of the diverse (group) beam search with finished-hypothesis pools (valor_beam_group_step; the law: include/valor_hip.h,
// restated on the host by valor_amd.decode.beam_group_step_host). The beam of K slots is G groups of Kg = K / G, each with its own range
// of the pool; the groups of a sample are searched ONE AFTER ANOTHER inside the launch, and a later group orders its candidates by
// a = c - pen[n_w], n_w = the number of new open slots that earlier groups filled with word w at this step (Vijayakumar et al., Hamming
// diversity on the current step's words). The penalty steers the SELECTION only: a slot, a pool offer and the early-exit bound carry the
// unpenalised c, so scores stay true log-probabilities (HF-style implementations fold the penalty into the running score).
//   One 1024-thread workgroup per sample, as beam_pool_step_kernel (beam_pool.hip), per group: the threads scan the group's rows (one row
//   at step 0), every thread keeping the best KMAX >= 2 Kg keys of its stride in registers (its candidates arrive in index order, so a
//   strict comparison keeps equal keys in index order); since pen >= 0, a <= c, and only a candidate whose c passes the list's tail pays
//   for n_w, a count over the <= 8 words in LDS that the earlier groups took. Then up to 2 Kg rounds of a workgroup-wide arg max over
//   the threads' heads; the threads rho < 2 Kg recompute the unpenalised c of the taken candidates (the same fp32 operations, the same
//   bits); thread 0 walks them and leaves the new slots, the pool's row writes and the taken words in LDS. After the last group all
//   threads copy the history rows and the pool rows. No atomics, no workspace, every reduction has a fixed order, global memory is
//   written with vector stores, every parameter by value: the result is a pure function of the inputs.
#include "common.h"

#define BG_THREADS 1024
#define BG_MAXK 8
#define BG_NONE 0x7fffffff

DEVINL bool bg_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

template <int KMAX>
__global__ __launch_bounds__(BG_THREADS) void beam_group_step_kernel(
    const float* __restrict__ logits, int64_t ld, int64_t rs_s, int64_t rs_k, const float* __restrict__ lse,
    const float* __restrict__ scores_in, const int64_t* __restrict__ hist_in, const float* __restrict__ inv_len,
    const float* __restrict__ pen, int b, int cur, int V, int K, int G, int L, int t, int eos, float floor, int alpha_pos, int early,
    float* __restrict__ scores_out, int64_t* __restrict__ hist_out, int64_t* __restrict__ tok, int64_t* __restrict__ parent,
    uint8_t* __restrict__ active, int64_t* __restrict__ pool_seq, float* __restrict__ pool_logprob, float* __restrict__ pool_rank,
    int32_t* __restrict__ pool_len, int32_t* __restrict__ pool_ins, int32_t* __restrict__ pool_cnt, uint8_t* __restrict__ gdone,
    uint8_t* __restrict__ done) {
    __shared__ float wv[16];
    __shared__ int wi[16];
    __shared__ int sel_i[2 * BG_MAXK];                       // the taken candidates of the group, in rank order
    __shared__ float sel_c[2 * BG_MAXK];                     // ... and their unpenalised scores
    __shared__ float slot_sc[BG_MAXK];                       // the new slots, all groups
    __shared__ int slot_par[BG_MAXK], slot_tok[BG_MAXK], slot_act[BG_MAXK], slot_keep[BG_MAXK];
    __shared__ float p_rank[BG_MAXK];                        // the group's pool range while thread 0 updates it
    __shared__ int p_ins[BG_MAXK];
    __shared__ int off_dst[2 * BG_MAXK], off_par[2 * BG_MAXK], off_tok[2 * BG_MAXK];   // pool rows to write: entry, parent slot, last word
    __shared__ int took[BG_MAXK];                            // the words of the new open slots so far
    __shared__ int n_off, n_took;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t sK = (int64_t)s * K;
    const int Kg = K / G;
    if (done[s]) {                                           // frozen (workgroup-uniform)
        for (int i = tid; i < K * L; i += BG_THREADS) hist_out[sK * L + i] = hist_in[sK * L + i];
        if (tid < K) {
            scores_out[sK + tid] = scores_in[sK + tid];
            tok[(int64_t)tid * b + s] = eos;
            parent[(int64_t)tid * b + s] = (int64_t)tid * b + s;
            active[(int64_t)tid * b + s] = 0;
        }
        return;
    }
    if (tid == 0) { n_off = 0; n_took = 0; }
    __syncthreads();
    bool all_done = true;                                    // (thread 0's copy is the one that counts)
    for (int g = 0; g < G; ++g) {
        const int lo = g * Kg;
        if (gdone[(int64_t)s * G + g]) {                     // a done group is frozen and lends no words (workgroup-uniform)
            if (tid < Kg) {
                slot_sc[lo + tid] = scores_in[sK + lo + tid];
                slot_par[lo + tid] = lo + tid; slot_tok[lo + tid] = eos; slot_act[lo + tid] = 0; slot_keep[lo + tid] = 1;
            }
            continue;
        }
        const int ntk = n_took;
        float lv[KMAX];
        int li[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) { lv[j] = -INFINITY; li[j] = BG_NONE; }
        const int kbeg = cur == 1 ? 0 : lo, kend = cur == 1 ? 1 : lo + Kg;     // step 0: every group reads the one row of slot 0
        for (int k = kbeg; k < kend; ++k) {
            const float sl = scores_in[sK + k];
            if (!(sl > -INFINITY)) continue;                 // a dead slot supplies no candidates
            const int64_t row = (int64_t)s * rs_s + (int64_t)k * rs_k;
            const float* x = logits + row * ld;
            const float l = lse[row];
            for (int w0 = tid; w0 < V; w0 += 4 * BG_THREADS) {      // four loads in flight (the insertion below is a dependent chain)
                float xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) xv[u] = w0 + u * BG_THREADS < V ? x[w0 + u * BG_THREADS] : 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int w = w0 + u * BG_THREADS;
                    const float c = sl + (xv[u] - l);
                    if (w < V && xv[u] > floor && c > lv[KMAX - 1]) {          // a <= c: nothing below the tail needs its count
                        int n = 0;
                        for (int j = 0; j < ntk; ++j) n += took[j] == w ? 1 : 0;
                        const float a = c - pen[n];                            // (pen[0] = 0; -inf and NaN never pass)
                        if (a > lv[KMAX - 1]) {
                            lv[KMAX - 1] = a; li[KMAX - 1] = k * V + w;
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
        }
        int n_sel = 0;                                       // (the same in every thread)
        for (int r = 0; r < 2 * Kg; ++r) {
            float bv = lv[0];
            int bi = li[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (bg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
            __syncthreads();
            bv = wv[0]; bi = wi[0];
#pragma unroll
            for (int j = 1; j < 16; ++j)
                if (bg_better(wv[j], wi[j], bv, bi)) { bv = wv[j]; bi = wi[j]; }
            __syncthreads();
            if (bi == BG_NONE) break;                        // nothing above -inf is left
            if (li[0] == bi) {                               // this thread's head won: pop it
#pragma unroll
                for (int j = 0; j + 1 < KMAX; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; }
                lv[KMAX - 1] = -INFINITY; li[KMAX - 1] = BG_NONE;
            }
            if (tid == 0) sel_i[r] = bi;
            n_sel = r + 1;
        }
        __syncthreads();
        if (tid < n_sel) {                                   // the unpenalised score of a taken candidate: the scan's own operations
            const int k = sel_i[tid] / V, w = sel_i[tid] - k * V;
            const int64_t row = (int64_t)s * rs_s + (int64_t)k * rs_k;
            sel_c[tid] = scores_in[sK + k] + (logits[row * ld + w] - lse[row]);
        }
        __syncthreads();
        if (tid == 0) {
            const int64_t cnt = ((int64_t)s * G + g) * 2;
            int pn = pool_cnt[cnt], pnext = pool_cnt[cnt + 1];
            pn = pn < 0 ? 0 : (pn > Kg ? Kg : pn);
            for (int j = 0; j < pn; ++j) { p_rank[j] = pool_rank[sK + lo + j]; p_ins[j] = pool_ins[sK + lo + j]; }
            int filled = 0, noff = n_off, nt = ntk;
            float top = -INFINITY;                           // the largest new score of the group
            for (int rho = 0; rho < n_sel && filled < Kg; ++rho) {
                const float c = sel_c[rho];
                const int k = sel_i[rho] / V, w = sel_i[rho] - k * V;
                const bool ends = w == eos;
                if (ends && rho >= Kg) continue;
                if (!ends) {
                    slot_sc[lo + filled] = c; slot_par[lo + filled] = k; slot_tok[lo + filled] = w; ++filled;
                    took[nt++] = w;
                    top = c > top ? c : top;
                }
                if (!ends && t < L - 1) continue;
                const int len = ends ? t + 1 : L;
                const float rank = c * inv_len[len];
                int dst = -1;
                if (pn < Kg) dst = pn++;
                else {
                    int worst = 0;
                    for (int j = 1; j < Kg; ++j)
                        if (p_rank[j] < p_rank[worst] || (p_rank[j] == p_rank[worst] && p_ins[j] > p_ins[worst])) worst = j;
                    if (rank > p_rank[worst]) dst = worst;
                }
                if (dst >= 0) {
                    const int64_t e = sK + lo + dst;
                    p_rank[dst] = rank; p_ins[dst] = pnext;
                    pool_logprob[e] = c; pool_rank[e] = rank; pool_len[e] = len; pool_ins[e] = pnext;
                    ++pnext;
                    off_dst[noff] = lo + dst; off_par[noff] = k; off_tok[noff] = w; ++noff;
                }
            }
            for (int j = filled; j < Kg; ++j) { slot_sc[lo + j] = -INFINITY; slot_par[lo + j] = lo + j; slot_tok[lo + j] = eos; }
            bool d = true;
            if (t < L - 1) {
                d = filled == 0;
                if (!d && pn == Kg) {
                    if (early) d = true;
                    else {
                        float worst = p_rank[0];
                        for (int j = 1; j < Kg; ++j) worst = p_rank[j] < worst ? p_rank[j] : worst;
                        const float bound = top * inv_len[alpha_pos ? L : t + 2];
                        d = worst >= bound;
                    }
                }
            }
            for (int j = 0; j < Kg; ++j) { slot_act[lo + j] = (!d && slot_sc[lo + j] > -INFINITY) ? 1 : 0; slot_keep[lo + j] = 0; }
            pool_cnt[cnt] = pn; pool_cnt[cnt + 1] = pnext;
            gdone[(int64_t)s * G + g] = d ? 1 : 0;
            all_done = all_done && d;
            n_off = noff; n_took = nt;
        }
        __syncthreads();
    }
    if (tid == 0) done[s] = all_done ? 1 : 0;
    __syncthreads();
    if (tid < K) {
        scores_out[sK + tid] = slot_sc[tid];
        tok[(int64_t)tid * b + s] = slot_tok[tid];
        parent[(int64_t)tid * b + s] = (int64_t)slot_par[tid] * b + s;
        active[(int64_t)tid * b + s] = slot_act[tid] ? 1 : 0;
    }
    for (int i = tid; i < K * L; i += BG_THREADS) {
        const int j = i / L, p = i - j * L;
        const int64_t v = (p == t && !slot_keep[j]) ? (int64_t)slot_tok[j] : hist_in[(sK + slot_par[j]) * L + p];
        hist_out[sK * L + i] = v;
    }
    const int no = n_off;
    for (int o = 0; o < no; ++o)                             // (an entry is rewritten by the same thread, in order)
        for (int p = tid; p < L; p += BG_THREADS) {
            const int64_t v = p < t ? hist_in[(sK + off_par[o]) * L + p] : (p == t ? (int64_t)off_tok[o] : (int64_t)eos);
            pool_seq[(sK + off_dst[o]) * L + p] = v;
        }
}

#define BG_LAUNCH(KMAX)                                                                                                                  \
    hipLaunchKernelGGL((beam_group_step_kernel<KMAX>), dim3((unsigned)b), dim3(BG_THREADS), 0, st, logits, ld, row_stride_s, row_stride_k, \
                       lse, scores_in, hist_in, inv_len, pen, b, cur, V, beam, groups, max_len, t, (int)eos, floor, alpha_pos,            \
                       early_stopping, scores_out, hist_out, tok, parent, active, pool_seq, pool_logprob, pool_rank, pool_len, pool_ins, \
                       pool_cnt, gdone, done)

extern "C" int valor_beam_group_step(void* stream, const float* logits, int64_t ld, int64_t row_stride_s, int64_t row_stride_k,
                                     const float* lse, const float* scores_in, const int64_t* hist_in, const float* inv_len,
                                     const float* pen, int b, int cur, int V, int beam, int groups, int max_len, int t, int64_t eos,
                                     float floor, int alpha_pos, int early_stopping, float* scores_out, int64_t* hist_out, int64_t* tok,
                                     int64_t* parent, uint8_t* active, int64_t* pool_seq, float* pool_logprob, float* pool_rank,
                                     int32_t* pool_len, int32_t* pool_ins, int32_t* pool_cnt, uint8_t* gdone, uint8_t* done) {
    if (b == 0) return VALOR_OK;
    if (!logits || !lse || !scores_in || !hist_in || !inv_len || !pen || !scores_out || !hist_out || !tok || !parent || !active ||
        !pool_seq || !pool_logprob || !pool_rank || !pool_len || !pool_ins || !pool_cnt || !gdone || !done || hist_in == hist_out)
        return VALOR_ERR_ARG;
    if (b < 0 || beam < 1 || beam > BG_MAXK || groups < 1 || groups > beam || beam % groups || (cur != 1 && cur != beam) || V < 1 ||
        ld < V || row_stride_s < 0 || row_stride_k < 0)
        return VALOR_ERR_ARG;
    const int kg = beam / groups;
    if (V < 2 * kg || (int64_t)cur * V < 2 * beam || (int64_t)cur * V >= 0x7fffffff || max_len < 1 || max_len > 512 || t < 0 || t >= max_len || eos < 0 || eos >= V ||
        floor != floor)
        return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (kg == 1) BG_LAUNCH(2);
    else if (kg == 2) BG_LAUNCH(4);
    else if (kg <= 4) BG_LAUNCH(8);
    else BG_LAUNCH(16);
    return valor_launch_status();
}
