// One step of the sampled caption decode (VALOR.decode_greedy with mode 'sample', model/pretrain.py:1007-1020): a categorical draw from
// softmax(logits) per row, the log-probability of the drawn token and the [SEP] bookkeeping, in one launch.
//   Draw: Gumbel-max. w* = argmax_w (z_w + g_w), g_w = -log(-log u_w), u_w i.i.d. uniform on (0, 1): P(w* = w) = softmax(z)_w (up to the
//     2^-24 grid of u below).
//     u_w comes from Philox4x32-10(seed, offset + r * ceil(V / 4) + w / 4), word w % 4, as (x >> 9) * 2^-23 + 2^-24: the odd multiples
//     of 2^-24 in (0, 1), every one exact in fp32 (the largest, 1 - 2^-24, is representable: u is never 1, -log u never 0, no key is +inf). Ties go to the lower index. The draw is a pure function of (seed, offset, r, w, logits): graph replay and eager
//     issue give the same tokens, and nothing is atomic.
//   The same pass keeps the row's running max / sum of exp (online log-sum-exp): logP = z[w*] - lse.
//   A row whose `unfinished` flag is 0 writes [SEP] and logP 0 without reading its logits. A row that drew [SEP] finishes. A row with a
//   NaN logit (or with no finite logit) writes [SEP], logP NaN, and finishes: every written token is an index in [0, V).
// One 1024-thread workgroup per row (a decoding step has only b rows: sixteen waves per CU hide the latency of the per-element Philox and
// transcendental chains), fp32 statistics. The draw does not depend on the reduction order; the log-sum-exp's rounding does.
#include "common.h"

#define SAMPLE_THREADS 1024

struct SampleAcc {
    float m, s;        // running max and sum of exp(z - m)
    float key;         // best z + g so far
    int idx;           // its column (INT_MAX: none)
    int nan;
};

DEVINL void acc_lse(SampleAcc& a, float m2, float s2) {
    if (m2 == -INFINITY) return;
    if (a.m == -INFINITY) { a.m = m2; a.s = s2; return; }
    if (m2 > a.m) { a.s = a.s * expf(a.m - m2) + s2; a.m = m2; }
    else a.s += s2 * expf(m2 - a.m);
}
DEVINL void acc_key(SampleAcc& a, float k2, int i2) {
    if (k2 > a.key || (k2 == a.key && i2 < a.idx)) { a.key = k2; a.idx = i2; }
}
DEVINL void acc_one(SampleAcc& a, float z, uint32_t bits, int w) {
    if (z != z) { a.nan = 1; return; }
    if (z == -INFINITY) return;
    // online log-sum-exp: one exp per element
    if (z > a.m) { a.s = (a.m == -INFINITY ? 0.f : a.s * expf(a.m - z)) + 1.f; a.m = z; }
    else a.s += expf(z - a.m);
    const float u = (float)(bits >> 9) * 1.1920928955078125e-7f + 5.9604644775390625e-8f;      // (x >> 9) 2^-23 + 2^-24, exact
    acc_key(a, z - logf(-logf(u)), w);
}
DEVINL void acc_merge(SampleAcc& a, const SampleAcc& b) {
    acc_lse(a, b.m, b.s);
    acc_key(a, b.key, b.idx);
    a.nan |= b.nan;
}
DEVINL SampleAcc acc_shfl(const SampleAcc& a, int o) {
    SampleAcc b;
    b.m = __shfl_xor(a.m, o, 64);
    b.s = __shfl_xor(a.s, o, 64);
    b.key = __shfl_xor(a.key, o, 64);
    b.idx = __shfl_xor(a.idx, o, 64);
    b.nan = __shfl_xor(a.nan, o, 64);
    return b;
}

template <bool VEC>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_tokens_kernel(const float* __restrict__ logits, int64_t ld, int V, uint64_t seed,
                                                                     uint64_t offset, int64_t eos, uint8_t* __restrict__ unfinished,
                                                                     int64_t* __restrict__ tok, int64_t* __restrict__ sents, int64_t sents_ld,
                                                                     float* __restrict__ logprobs, int64_t lp_ld) {
    __shared__ SampleAcc red[SAMPLE_THREADS / WAVE];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!unfinished[r]) {                      // finished earlier: [SEP], logP 0 (reward_loss masks these positions)
        if (tid == 0) {
            tok[r] = eos;
            sents[(int64_t)r * sents_ld] = eos;
            logprobs[(int64_t)r * lp_ld] = 0.f;
        }
        return;
    }
    const float* x = logits + (int64_t)r * ld;
    const int G = (V + 3) >> 2;
    const uint64_t ctr0 = offset + (uint64_t)r * (uint64_t)G;
    SampleAcc a;
    a.m = -INFINITY; a.s = 0.f; a.key = -INFINITY; a.idx = 0x7fffffff; a.nan = 0;
    for (int c = tid; c < G; c += SAMPLE_THREADS) {
        const Philox4 p = philox4x32_10(seed, ctr0 + (uint64_t)c);
        const int w0 = c * 4;
        const uint32_t b0 = p.v[0], b1 = p.v[1], b2 = p.v[2], b3 = p.v[3];
        if (VEC && w0 + 4 <= V) {
            const f32x4_t z = *(const f32x4_t*)(x + w0);
            acc_one(a, z[0], b0, w0);
            acc_one(a, z[1], b1, w0 + 1);
            acc_one(a, z[2], b2, w0 + 2);
            acc_one(a, z[3], b3, w0 + 3);
        } else {
            if (w0 < V) acc_one(a, x[w0], b0, w0);
            if (w0 + 1 < V) acc_one(a, x[w0 + 1], b1, w0 + 1);
            if (w0 + 2 < V) acc_one(a, x[w0 + 2], b2, w0 + 2);
            if (w0 + 3 < V) acc_one(a, x[w0 + 3], b3, w0 + 3);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc_merge(a, acc_shfl(a, o));
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (tid == 0) {
        SampleAcc t = red[0];
#pragma unroll
        for (int k = 1; k < SAMPLE_THREADS / WAVE; ++k) acc_merge(t, red[k]);
        int64_t w;
        float lp;
        bool fin;
        if (t.nan || t.idx < 0 || t.idx >= V) {
            w = eos; lp = NAN; fin = true;
        } else {
            w = t.idx;
            lp = x[w] - (t.m + logf(t.s));
            fin = w == eos;
        }
        tok[r] = w;
        sents[(int64_t)r * sents_ld] = w;
        logprobs[(int64_t)r * lp_ld] = lp;
        if (fin) unfinished[r] = 0;
    }
}

extern "C" int valor_sample_tokens(void* stream, const float* logits, int64_t ld, int R, int V, uint64_t seed, uint64_t offset, int64_t eos,
                                   uint8_t* unfinished, int64_t* tok, int64_t* sents, int64_t sents_ld, float* logprobs, int64_t lp_ld) {
    if (!logits || !unfinished || !tok || !sents || !logprobs) return VALOR_ERR_ARG;
    if (R <= 0 || V <= 0 || ld < V || eos < 0 || eos >= V || sents_ld < 0 || lp_ld < 0) return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (ld % 4 == 0 && ((uintptr_t)logits & 15) == 0)
        hipLaunchKernelGGL((sample_tokens_kernel<true>), dim3(R), dim3(SAMPLE_THREADS), 0, st, logits, ld, V, seed, offset, eos, unfinished, tok,
                           sents, sents_ld, logprobs, lp_ld);
    else
        hipLaunchKernelGGL((sample_tokens_kernel<false>), dim3(R), dim3(SAMPLE_THREADS), 0, st, logits, ld, V, seed, offset, eos, unfinished, tok,
                           sents, sents_ld, logprobs, lp_ld);
    return valor_launch_status();
}

// ---------------------------------------------------------------------------------------------
// out = sum_r w[r] * x[r] / n  (the forward of the reward-weighted caption loss, pretrain.py:166-173: mean over the labelled positions of
// -logP * reward); one workgroup, no host sync
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weighted_mean_f32_kernel(const float* x, const float* w, int64_t n, float* out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += w[i] * x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = (red[0] + red[1] + red[2] + red[3]) / (float)n;
}
extern "C" int valor_weighted_mean_f32(void* stream, const float* x, const float* w, int64_t n, float* out) {
    if (n <= 0 || !x || !w || !out) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(weighted_mean_f32_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, w, n, out);
    return valor_launch_status();
}
