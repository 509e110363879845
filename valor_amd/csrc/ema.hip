// Exponential moving average of the weights over the flat fp32 master arena (valor_amd/ema.py WeightEMA): one streaming launch and a
// one-thread launch that advances the device count, the way adamw_count_kernel follows adamw_kernel.
//
// The law, per element, in fp32, every named operation rounded once (fp contract(off) below: nothing is contracted into an fma, so a host
// restatement in plain fp32 tensor operations is bit-equal -- ema.ema_host):
//   k = *count                                               updates applied so far
//   d = warmup ? min(decay, (1 + k) / (10 + k)) : decay      one IEEE division of two converted integers (exact below 2^24)
//   a = 1 - d ;  t = w - ema ;  ema = ema + a * t            a product, then a sum
// A parameter that never moves (w == ema) has t = 0 and stays exactly where it is, whatever d.
// A non-finite *gscale_dev (the optimizer skipped the step, optim.hip) writes nothing and leaves the count: the same test as the update
// kernel's. k and the skip are known to the device only; nothing is read back.
//
// HBM-bound at 12 B per element (read w, read ema, write ema). 16 bytes per lane, two vectors per thread and iteration in flight, as
// adamw_kernel; NT bit 0: non-temporal loads, bit 1: non-temporal stores (A/B hook; the default is what tools/ema_bench.py measured).
#include "common.h"
#include <stdlib.h>

// hipcc contracts by default, and the __f*_rn intrinsics do not stop it: they are inline functions of the HIP headers, compiled under the
// headers' contraction state, and __fadd_rn(e, __fmul_rn(a, t)) came out as v_pk_fma_f32. So: plain operators, contraction off for the
// whole file. The division's expansion is the backend's and stays correctly rounded.
#pragma clang fp contract(off)

#define EMA_THREADS 256
#define EMA_UNROLL 2

DEVINL float ema_decay_at(float decay, int warmup, int32_t k) {
    if (!warmup) return decay;
    const float q = (float)(1 + (int64_t)k) / (float)(10 + (int64_t)k);
    return fminf(decay, q);
}

DEVINL float ema_one(float w, float e, float a) {
    const float t = w - e;
    const float p = a * t;
    return e + p;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_kernel(const float* __restrict__ w, float* __restrict__ ema, int64_t n, float decay,
                                                          int warmup, const int32_t* count, const float* gscale_dev, int nt) {
    if (gscale_dev && !(fabsf(*gscale_dev) < INFINITY)) return;         // skipped step: nothing is written
    const float a = 1.0f - ema_decay_at(decay, warmup, *count);
    const bool ntl = (nt & 1) != 0, nts = (nt & 2) != 0;
    const int64_t nvec = n >> 2;                                         // whole 16-byte vectors; the last n & 3 elements are the tail
    const int64_t stride = (int64_t)gridDim.x * EMA_THREADS;
    for (int64_t v0 = (int64_t)blockIdx.x * EMA_THREADS + threadIdx.x; v0 < nvec; v0 += EMA_UNROLL * stride) {
        f32x4_t x[EMA_UNROLL], e[EMA_UNROLL];
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) {
            const int64_t v = v0 + u * stride;
            if (v >= nvec) continue;
            x[u] = ntl ? __builtin_nontemporal_load((const f32x4_t*)w + v) : ((const f32x4_t*)w)[v];
            e[u] = ntl ? __builtin_nontemporal_load((const f32x4_t*)ema + v) : ((const f32x4_t*)ema)[v];
        }
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) {
            const int64_t v = v0 + u * stride;
            if (v >= nvec) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) e[u][k] = ema_one(x[u][k], e[u][k], a);
            if (nts) __builtin_nontemporal_store(e[u], (f32x4_t*)ema + v); else ((f32x4_t*)ema)[v] = e[u];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                      // tail: at most three elements, one lane each
        const int64_t i = (nvec << 2) + threadIdx.x;
        ema[i] = ema_one(w[i], ema[i], a);
    }
}

// behind ema_kernel in stream order: every element has read k by now
__global__ void ema_count_kernel(int32_t* count, const float* gscale_dev) {
    if (gscale_dev && !(fabsf(*gscale_dev) < INFINITY)) return;
    *count += 1;
}

static int g_ema_nt = [] { const char* e = getenv("VALOR_EMA_NT"); return e ? atoi(e) : 0; }();
// non-temporal accesses of the EMA kernel (bit 0 loads, bit 1 stores); returns the previous value, v < 0 only queries
extern "C" int valor_ema_set_nt(int v) { const int o = g_ema_nt; if (v >= 0) g_ema_nt = v & 3; return o; }

extern "C" int valor_ema_update(void* stream, const float* w, float* ema, int64_t n, float decay, int warmup, int32_t* count,
                                const float* gscale_dev) {
    if (!w || !ema || !count || n <= 0 || !(decay >= 0.0f && decay <= 1.0f)) return VALOR_ERR_ARG;      // (a NaN decay fails both compares)
    if (((uintptr_t)w & 15) || ((uintptr_t)ema & 15) || ((uintptr_t)count & 3) || ((uintptr_t)gscale_dev & 3)) return VALOR_ERR_ARG;
    if ((uintptr_t)w < (uintptr_t)(ema + n) && (uintptr_t)ema < (uintptr_t)(w + n)) return VALOR_ERR_ARG;   // overlapping buffers
    const int64_t nvec = n >> 2;
    int64_t blocks = (nvec + EMA_UNROLL * EMA_THREADS - 1) / (EMA_UNROLL * EMA_THREADS);
    blocks = blocks < 1 ? 1 : blocks > 8192 ? 8192 : blocks;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)blocks), dim3(EMA_THREADS), 0, st, w, ema, n, decay, warmup != 0, count, gscale_dev, g_ema_nt);
    int rc = valor_launch_status();
    if (rc != VALOR_OK) return rc;
    hipLaunchKernelGGL(ema_count_kernel, dim3(1), dim3(1), 0, st, count, gscale_dev);
    return valor_launch_status();
}
