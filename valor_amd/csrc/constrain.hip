// Generation controls of one decoding step (valor_logits_constrain; the law: include/valor_hip.h): repetition penalty, no repeated
// n-gram, minimum length and a list of suppressed tokens, applied in place to the step's fp32 logits rows from each row's own generated
// tokens. One launch between the decoding step and the selection (arg max, valor_beam_select, the samplers); it sits outside the
// captured step and takes every parameter by value, so a kept session serves any setting.
//   History addressing: the kernel takes the two strides the way valor_beam_select takes row_stride_s / row_stride_k. Row r reads
//     hist + (r % b) * hist_stride_s + (r / b) * hist_stride_k, t tokens with unit stride. Beam search keeps its words as
//     [b, beam, max_len] (sample, beam) while the decoder's rows are beam-major (r = k * b + s): hist_stride_s = beam * max_len,
//     hist_stride_k = max_len and nothing is re-gathered for this kernel. A row-ordered history is b = R, hist_stride_k = 0.
//   One 256-thread workgroup per row. The history (t <= 512 tokens: the position table of the decoder has at most 512 rows) is copied
//   to LDS once; the distinct-token test of rule 1 (thread i owns position i and acts only when no earlier position holds the same
//   token: every column is rewritten by exactly one thread, exactly once) and the n-gram match of rule 2 (thread i compares the n - 1
//   tokens at i with the last n - 1) are scans of that copy. A barrier separates the read-modify-write of rule 1 from the -inf stores
//   of rules 2-4: a banned column is -inf whatever rule 1 did to it. The -inf stores of several threads to one column carry the same
//   bits. No atomics, no workspace: the result is a pure function of the inputs, however the threads split the history.
#include "common.h"

#define CONSTRAIN_THREADS 256
#define CONSTRAIN_MAX_T 512

__global__ __launch_bounds__(CONSTRAIN_THREADS) void logits_constrain_kernel(float* __restrict__ logits, int64_t ld, int V,
                                                                           const int64_t* __restrict__ hist, int64_t hist_stride_s,
                                                                           int64_t hist_stride_k, int b, int t, int64_t eos, float penalty,
                                                                           float inv_penalty, int ngram, int min_len,
                                                                           const int32_t* __restrict__ suppress, int n_suppress,
                                                                           const uint8_t* __restrict__ active) {
    __shared__ int64_t h[CONSTRAIN_MAX_T];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (active && !active[r]) return;                  // (workgroup-uniform)
    float* z = logits + (int64_t)r * ld;
    if (t > 0) {
        const int64_t* src = hist + (int64_t)(r % b) * hist_stride_s + (int64_t)(r / b) * hist_stride_k;
        for (int i = tid; i < t; i += CONSTRAIN_THREADS) h[i] = src[i];
    }
    __syncthreads();
    // rule 1: every distinct token of the history once -- at its first occurrence
    if (penalty != 1.f) {
        for (int i = tid; i < t; i += CONSTRAIN_THREADS) {
            const int64_t w = h[i];
            if (w < 0 || w >= V) continue;
            bool first = true;
            for (int j = 0; j < i; ++j) first = first && h[j] != w;
            if (!first) continue;
            const float x = z[w];
            z[w] = x > 0.f ? x * inv_penalty : x * penalty;
        }
    }
    __threadfence_block();
    __syncthreads();
    // rule 2: the tokens that followed an earlier occurrence of the last n - 1 tokens
    if (ngram >= 1 && t >= ngram - 1) {
        const int m = ngram - 1, tail = t - m;
        for (int i = tid; i + ngram <= t; i += CONSTRAIN_THREADS) {
            bool same = true;
            for (int j = 0; j < m; ++j) same = same && h[i + j] == h[tail + j];
            const int64_t w = h[i + m];
            if (same && w >= 0 && w < V) z[w] = -INFINITY;
        }
    }
    // rule 3
    if (tid == 0 && t < min_len) z[eos] = -INFINITY;
    // rule 4
    for (int i = tid; i < n_suppress; i += CONSTRAIN_THREADS) {
        const int32_t w = suppress[i];
        if (w >= 0 && w < V) z[w] = -INFINITY;
    }
}

extern "C" int valor_logits_constrain(void* stream, float* logits, int64_t ld, int R, int V, const int64_t* hist, int64_t hist_stride_s,
                                      int64_t hist_stride_k, int b, int t, int64_t eos, float penalty, float inv_penalty, int ngram,
                                      int min_len, const int32_t* suppress, int n_suppress, const uint8_t* active) {
    if (R == 0) return VALOR_OK;
    if (!logits || R < 0 || V < 1 || ld < V || t < 0 || t > CONSTRAIN_MAX_T || (!hist && t > 0)) return VALOR_ERR_ARG;
    if (b < 1 || hist_stride_s < 0 || hist_stride_k < 0) return VALOR_ERR_ARG;
    if (ngram < 0 || min_len < 0 || eos < 0 || eos >= V) return VALOR_ERR_ARG;
    if (!(penalty > 0.f) || !(penalty < INFINITY)) return VALOR_ERR_ARG;
    if (n_suppress < 0 || (!suppress && n_suppress > 0)) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(logits_constrain_kernel, dim3(R), dim3(CONSTRAIN_THREADS), 0, (hipStream_t)stream, logits, ld, V, hist, hist_stride_s,
                       hist_stride_k, b, t, eos, penalty, inv_penalty, ngram, min_len, suppress, n_suppress, active);
    return valor_launch_status();
}
