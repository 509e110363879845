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
// The filtered draw (valor_sample_tokens_filtered): temperature, top-k, then top-p over what top-k left, ties at a threshold kept; the
// draw itself is the kernel above on the row where(w in S, y_w, -inf), y = logits * inv_temperature (the law: include/valor_hip.h).
//   Both thresholds are order statistics of the row and are found by radix select on order-preserving uint32 keys of y: three passes
//   (11 + 11 + 10 key bits), each a 2048-bin histogram in LDS and a descending scan for the bin in which the running weight reaches the
//   target. The weight of a column is 1 (top-k: the target is k) or the fixed-point mass floor(exp(y - max y) * 2^40) (top-p: the target
//   is ceil(top_p * total)). Histograms are built with 64-bit INTEGER LDS atomics: sums of integers do not depend on their order, so the
//   thresholds -- and with them the draw -- are a pure function of the row, whatever the thread split. No float atomic anywhere.
//   Mass error: truncation < 2^-40 per column (V < 2^16 columns: the total stays below 2^56 and 4.5e-8 of the leader's mass), expf 1 ulp,
//   the rounding of y - max below 3e-8 of a column's mass: the compared ratio is within 1e-6 of its exact value.
//   The row is re-read from global memory by every pass (a 30522-float row is 119 KiB, 64 rows are L2-resident); the last pass is the
//   unfiltered kernel's loop with the columns outside S skipped: with every filter off it gives that kernel's bits.
// ---------------------------------------------------------------------------------------------
#define SF_BINS 2048
#define SF_FLOOR 0x00800000u            // the smallest key above key(-inf) = 0x007fffff: "every column with y > -inf"

struct FilterShared {
    unsigned long long hist[SF_BINS];
    unsigned long long wsum[SAMPLE_THREADS / WAVE];
    unsigned long long acc;
    uint32_t prefix, maxkey, minkey;
    int nfin, nan, kept;
    SampleAcc red[SAMPLE_THREADS / WAVE];
};

// order-preserving key of a non-NaN float (-0 counts as +0: the law compares values)
DEVINL uint32_t sf_key(float y) {
    uint32_t u = __float_as_uint(y);
    if ((u << 1) == 0) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// y = logit * inv_temperature: ONE rounded fp32 multiply wherever it is used (never contracted into a later subtraction)
DEVINL float sf_scale(float z, float inv) {
#pragma clang fp contract(off)
    return z * inv;
}
DEVINL float sf_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
DEVINL unsigned long long sf_mass(float y, float ymax) {
    const float e = y == ymax ? 1.f : expf(y - ymax);
    return (unsigned long long)(e * 1099511627776.f);          // 2^40: exact scaling, truncated
}

// f(y, w) for every column w of the row this thread owns (the 4-column groups c = tid, tid + 1024, ...), y = x[w] * inv
template <bool VEC, typename F>
DEVINL void sf_columns(const float* __restrict__ x, int V, float inv, int tid, F f) {
    const int G = (V + 3) >> 2;
    for (int c = tid; c < G; c += SAMPLE_THREADS) {
        const int w0 = c * 4;
        if (VEC && w0 + 4 <= V) {
            const f32x4_t z = *(const f32x4_t*)(x + w0);
            f(sf_scale(z[0], inv), w0);
            f(sf_scale(z[1], inv), w0 + 1);
            f(sf_scale(z[2], inv), w0 + 2);
            f(sf_scale(z[3], inv), w0 + 3);
        } else {
            for (int w = w0; w < w0 + 4 && w < V; ++w) f(sf_scale(x[w], inv), w);
        }
    }
}

// the largest key K with weight{columns with key >= K and key >= lo} >= T (MASS: T = ceil(top_p * the total weight) instead).
// Every thread returns the same K. The caller guarantees a column with key >= lo and, when !MASS, 1 <= T <= their count.
template <bool VEC, bool MASS>
DEVINL uint32_t sf_select(FilterShared& sh, const float* __restrict__ x, int V, float inv, uint32_t lo, float ymax, unsigned long long T,
                          float top_p, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t prefix = 0;
    unsigned long long acc = 0;            // the weight of the keys above the prefix
    int prev_shift = 32;
#pragma unroll 1
    for (int p = 0; p < 3; ++p) {
        const int bits = p == 2 ? 10 : 11, shift = prev_shift - bits, nb = 1 << bits;
        for (int i = tid; i < SF_BINS; i += SAMPLE_THREADS) sh.hist[i] = 0;
        __syncthreads();
        sf_columns<VEC>(x, V, inv, tid, [&](float y, int) {
            const uint32_t k = sf_key(y);
            if (k < lo || (p > 0 && (k >> prev_shift) != prefix)) return;
            const unsigned long long wgt = MASS ? sf_mass(y, ymax) : 1ull;
            if (wgt) atomicAdd(&sh.hist[(k >> shift) & (uint32_t)(nb - 1)], wgt);
        });
        __syncthreads();
        // bins in descending order, two per thread: an exclusive scan over the workgroup
        const int d0 = 2 * tid, d1 = d0 + 1;
        const unsigned long long h0 = d0 < nb ? sh.hist[nb - 1 - d0] : 0ull, h1 = d1 < nb ? sh.hist[nb - 1 - d1] : 0ull;
        unsigned long long incl = h0 + h1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) sh.wsum[wave] = incl;
        __syncthreads();
        unsigned long long base = 0, total = 0;
#pragma unroll
        for (int k = 0; k < SAMPLE_THREADS / WAVE; ++k) {
            const unsigned long long v = sh.wsum[k];
            if (k < wave) base += v;
            total += v;
        }
        if (MASS && p == 0) {
            const double t = ceil((double)top_p * (double)total);
            T = t < 1.0 ? 1ull : (unsigned long long)t;
            if (T > total) T = total;
        }
        const unsigned long long ex = acc + base + incl - (h0 + h1);
        if (ex < T && T <= ex + h0) {
            sh.prefix = (prefix << bits) | (uint32_t)(nb - 1 - d0);
            sh.acc = ex;
        } else if (ex + h0 < T && T <= ex + h0 + h1) {
            sh.prefix = (prefix << bits) | (uint32_t)(nb - 1 - d1);
            sh.acc = ex + h0;
        }
        __syncthreads();
        prefix = sh.prefix;
        acc = sh.acc;
        prev_shift = shift;
    }
    return prefix;
}

template <bool VEC>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_tokens_filtered_kernel(const float* __restrict__ logits, int64_t ld, int V, uint64_t seed,
                                                                              uint64_t offset, int64_t eos, float inv, int top_k, float top_p,
                                                                              uint8_t* __restrict__ unfinished, int64_t* __restrict__ tok,
                                                                              int64_t* __restrict__ sents, int64_t sents_ld,
                                                                              float* __restrict__ logprobs, int64_t lp_ld,
                                                                              int32_t* __restrict__ kept, float* __restrict__ cut) {
    __shared__ FilterShared sh;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!unfinished[r]) {
        if (tid == 0) {
            tok[r] = eos;
            sents[(int64_t)r * sents_ld] = eos;
            logprobs[(int64_t)r * lp_ld] = 0.f;
            if (kept) kept[r] = 0;
            if (cut) cut[r] = NAN;
        }
        return;
    }
    const float* x = logits + (int64_t)r * ld;
    if (tid == 0) {
        sh.maxkey = 0u; sh.minkey = 0xffffffffu; sh.nfin = 0; sh.nan = 0; sh.kept = 0;
    }
    __syncthreads();
    {   // pass A: NaN anywhere, the number of columns above -inf, max y
        int nan = 0, nfin = 0;
        uint32_t mk = 0u;
        sf_columns<VEC>(x, V, inv, tid, [&](float y, int) {
            if (y != y) { nan = 1; return; }
            const uint32_t k = sf_key(y);
            nfin += k >= SF_FLOOR;
            mk = k > mk ? k : mk;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            nan |= __shfl_xor(nan, o, 64);
            nfin += __shfl_xor(nfin, o, 64);
            const uint32_t m2 = (uint32_t)__shfl_xor((int)mk, o, 64);
            mk = m2 > mk ? m2 : mk;
        }
        if (lane == 0) {
            if (nan) atomicOr(&sh.nan, 1);
            atomicAdd(&sh.nfin, nfin);
            atomicMax(&sh.maxkey, mk);
        }
    }
    __syncthreads();
    const int nfin = sh.nfin;
    const bool draws = !sh.nan && nfin > 0;            // (workgroup-uniform)
    uint32_t lo = SF_FLOOR;
    if (draws) {
        const float ymax = sf_unkey(sh.maxkey);
        if (top_k >= 1 && top_k < nfin) lo = sf_select<VEC, false>(sh, x, V, inv, lo, ymax, (unsigned long long)top_k, 1.f, tid);
        if (top_p < 1.f) lo = sf_select<VEC, true>(sh, x, V, inv, lo, ymax, 0ull, top_p, tid);
    }
    // the draw: valor_sample_tokens' loop over the columns of S
    const int G = (V + 3) >> 2;
    const uint64_t ctr0 = offset + (uint64_t)r * (uint64_t)G;
    SampleAcc a;
    a.m = -INFINITY; a.s = 0.f; a.key = -INFINITY; a.idx = 0x7fffffff; a.nan = 0;
    int nkept = 0;
    uint32_t mink = 0xffffffffu;
    auto one = [&](float z, uint32_t bits, int w) {
        const float y = sf_scale(z, inv);
        if (y != y) { a.nan = 1; return; }
        const uint32_t k = sf_key(y);
        if (k < lo) return;
        nkept += 1;
        mink = k < mink ? k : mink;
        acc_one(a, y, bits, w);
    };
    for (int c = tid; c < G; c += SAMPLE_THREADS) {
        const Philox4 p = philox4x32_10(seed, ctr0 + (uint64_t)c);
        const int w0 = c * 4;
        const uint32_t b0 = p.v[0], b1 = p.v[1], b2 = p.v[2], b3 = p.v[3];
        if (VEC && w0 + 4 <= V) {
            const f32x4_t z = *(const f32x4_t*)(x + w0);
            one(z[0], b0, w0);
            one(z[1], b1, w0 + 1);
            one(z[2], b2, w0 + 2);
            one(z[3], b3, w0 + 3);
        } else {
            if (w0 < V) one(x[w0], b0, w0);
            if (w0 + 1 < V) one(x[w0 + 1], b1, w0 + 1);
            if (w0 + 2 < V) one(x[w0 + 2], b2, w0 + 2);
            if (w0 + 3 < V) one(x[w0 + 3], b3, w0 + 3);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc_merge(a, acc_shfl(a, o));
        nkept += __shfl_xor(nkept, o, 64);
        const uint32_t m2 = (uint32_t)__shfl_xor((int)mink, o, 64);
        mink = m2 < mink ? m2 : mink;
    }
    if (lane == 0) {
        sh.red[wave] = a;
        atomicAdd(&sh.kept, nkept);
        atomicMin(&sh.minkey, mink);
    }
    __syncthreads();
    if (tid == 0) {
        SampleAcc t = sh.red[0];
#pragma unroll
        for (int k = 1; k < SAMPLE_THREADS / WAVE; ++k) acc_merge(t, sh.red[k]);
        int64_t w;
        float lp;
        bool fin;
        const bool bad = t.nan || t.idx < 0 || t.idx >= V;
        if (bad) {
            w = eos; lp = NAN; fin = true;
        } else {
            w = t.idx;
            lp = sf_scale(x[w], inv) - (t.m + logf(t.s));
            fin = w == eos;
        }
        tok[r] = w;
        sents[(int64_t)r * sents_ld] = w;
        logprobs[(int64_t)r * lp_ld] = lp;
        if (fin) unfinished[r] = 0;
        if (kept) kept[r] = bad ? 0 : sh.kept;
        if (cut) cut[r] = bad ? NAN : sf_unkey(sh.minkey);
    }
}

extern "C" int valor_sample_tokens_filtered(void* stream, const float* logits, int64_t ld, int R, int V, uint64_t seed, uint64_t offset,
                                            int64_t eos, float inv_temperature, int top_k, float top_p, uint8_t* unfinished, int64_t* tok,
                                            int64_t* sents, int64_t sents_ld, float* logprobs, int64_t lp_ld, int32_t* kept, float* cut) {
    if (R == 0) return VALOR_OK;
    if (!logits || !unfinished || !tok || !sents || !logprobs) return VALOR_ERR_ARG;
    if (R < 0 || V <= 0 || V > 65535 || ld < V || eos < 0 || eos >= V || sents_ld < 0 || lp_ld < 0 || top_k < 0) return VALOR_ERR_ARG;
    if (!(inv_temperature > 0.f) || !(inv_temperature < INFINITY) || !(top_p > 0.f) || !(top_p <= 1.f)) return VALOR_ERR_ARG;
    if (inv_temperature == 1.f && (top_k == 0 || top_k >= V) && top_p == 1.f && !kept && !cut)       // every filter off: the unfiltered kernel
        return valor_sample_tokens(stream, logits, ld, R, V, seed, offset, eos, unfinished, tok, sents, sents_ld, logprobs, lp_ld);
    hipStream_t st = (hipStream_t)stream;
    if (ld % 4 == 0 && ((uintptr_t)logits & 15) == 0)
        hipLaunchKernelGGL((sample_tokens_filtered_kernel<true>), dim3(R), dim3(SAMPLE_THREADS), 0, st, logits, ld, V, seed, offset, eos,
                           inv_temperature, top_k, top_p, unfinished, tok, sents, sents_ld, logprobs, lp_ld, kept, cut);
    else
        hipLaunchKernelGGL((sample_tokens_filtered_kernel<false>), dim3(R), dim3(SAMPLE_THREADS), 0, st, logits, ld, V, seed, offset, eos,
                           inv_temperature, top_k, top_p, unfinished, tok, sents, sents_ld, logprobs, lp_ld, kept, cut);
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
