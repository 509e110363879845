// Video patch dropout (FLIP / open_clip "patch dropout"; VideoMAE's tube masking when the subset is shared by a clip's frames): in
// training every frame keeps k of its Pn patches plus the class token, and everything behind the patch embedding runs on 1 + k rows.
//   - valor_patch_keep draws the subsets: patch p of draw group g = f / group has the 64-bit key w0 | w1 << 32 of
//     Philox4x32-10(seed, offset + *rng_base + g*Pn + p); the group keeps its k smallest keys, ties to the lower p -- the selection law of
//     masker.hip (the k smallest of i.i.d. keys are a uniform k-subset). Outputs: idx [N, k], the kept positions ascending, and
//     slot [N, Pn], its inverse (-1 = dropped). One wave per group, nothing atomic: a function of the arguments alone.
//   - valor_patchify_kept / valor_assemble_tokens_kept_fwd are valor_patchify / valor_assemble_tokens_fwd (misc.hip) on the kept rows
//     only, with the same arithmetic: their output equals the gathered rows of the full kernels bit for bit;
//   - valor_assemble_tokens_kept_bwd: dpatches = the rows of dout; dpos / dcls are sums over the frames in frame order through `slot`
//     (no atomics: deterministic; a position no frame kept gets exactly 0).
// A dropped patch is never read or written by any of them.
#include "common.h"

#define KEEP_MAX_PN 1024                       // ViT-L/14 at 336 px has 576 patches; one wave ranks a group by counting (Pn^2 / 64 per lane)

// grid = N / group blocks of one wave. Pass 1 leaves the group's keys in LDS; pass 2 ranks every position by a count over the group
// (rank < k: kept) and numbers the kept ones in position order (ballot + popcount prefix), then writes the rows of all the group's frames.
__global__ __launch_bounds__(64) void patch_keep_kernel(int Pn, int k, int group, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_base,
                                                        int32_t* __restrict__ idx, int32_t* __restrict__ slot) {
    __shared__ uint64_t keys[KEEP_MAX_PN];
    const int g = blockIdx.x, lane = threadIdx.x;
    const uint64_t ctr0 = rng_offset(offset, rng_base) + (uint64_t)g * (uint64_t)Pn;
    for (int p = lane; p < Pn; p += WAVE) {
        const Philox4 r = philox4x32_10(seed, ctr0 + (uint64_t)p);
        keys[p] = (uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32);
    }
    __syncthreads();
    const int64_t f0 = (int64_t)g * group;
    int base = 0;
    for (int c = 0; c < Pn; c += WAVE) {
        const int p = c + lane;
        bool kept = false;
        if (p < Pn) {
            const uint64_t key = keys[p];
            int rank = 0;
            for (int q = 0; q < Pn; ++q) {
                const uint64_t kq = keys[q];
                rank += (kq < key) | ((kq == key) & (q < p));
            }
            kept = rank < k;
        }
        const uint64_t bal = __ballot(kept);
        const int s = base + __popcll(bal & ((1ull << lane) - 1ull));
        base += __popcll(bal);
        if (p < Pn) {
            const bool wr = kept && s < k;     // the ranks are a permutation of 0 .. Pn-1, so exactly k positions are kept: s < k always holds
            for (int j = 0; j < group; ++j) {
                slot[(f0 + j) * Pn + p] = wr ? s : -1;
                if (wr) idx[(f0 + j) * k + s] = p;
            }
        }
    }
}

// valor_patchify's gather (misc.hip patchify_kernel) over the kept patches: output row f*k + j is patch idx[f, j] of image f.
template <typename T, int VEC>
__global__ void patchify_kept_kernel(const float* in, const int32_t* __restrict__ idx, T* out, int N, int C, int H, int W, int P, int k, int64_t ldo) {
    const int gh = H / P, gw = W / P, K = C * P * P;
    const int64_t totalv = (int64_t)N * k * K / VEC;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < totalv; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = q * VEC;
        const int kk = (int)(e % K);
        const int64_t row = e / K;
        const int n = (int)(row / k);
        const int p = min(max(idx[row], 0), gh * gw - 1);       // a table that is not valor_patch_keep's cannot read outside the image
        const int px = p % gw, py = p / gw;
        const int c = kk / (P * P), ij = kk % (P * P), i = ij / P, j = ij % P;   // j % VEC == 0 (P % VEC == 0)
        const float* src = in + (((int64_t)n * C + c) * H + (py * P + i)) * W + px * P + j;
        T* dst = out + row * ldo + kk;
        if constexpr (VEC == 4) store4<T>(dst, *(const f32x4_t*)src);
        else { dst[0] = from_f32<T>(src[0]); dst[1] = from_f32<T>(src[1]); }
    }
}

// out[f][0] = cls + pos[0] ; out[f][1 + j] = patches[f*k + j] (+ bias) + pos[1 + idx[f, j]], summed in assemble_fwd_kernel's order
template <typename T>
__global__ void assemble_kept_fwd_kernel(const T* patches, const T* cls, const T* pos, const T* bias, const int32_t* __restrict__ idx, T* out,
                                         int N, int Pn, int k, int E) {
    const int E4 = E / 4;
    const int64_t total = (int64_t)N * (k + 1) * E4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(q % E4) * 4;
        const int64_t r = q / E4;
        const int t = (int)(r % (k + 1));
        const int64_t n = r / (k + 1);
        f32x4_t v;
        if (t == 0) {
            v = load4<T>(pos + e);
            v += load4<T>(cls + e);
        } else {
            const int p = min(max(idx[n * k + (t - 1)], 0), Pn - 1);
            v = load4<T>(pos + (int64_t)(1 + p) * E + e);
            v += load4<T>(patches + (n * k + (t - 1)) * E + e);
            if (bias) v += load4<T>(bias + e);
        }
        store4<T>(out + r * E + e, v);
    }
}

// dpatches[f*k + j] = dout[f][1 + j]
template <typename T>
__global__ void assemble_kept_bwd_patches_kernel(const T* dout, T* dpatches, int N, int k, int E) {
    const int E4 = E / 4;
    const int64_t total = (int64_t)N * k * E4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(q % E4) * 4;
        const int64_t r = q / E4;
        const int j = (int)(r % k);
        const int64_t n = r / k;
        store4<T>(dpatches + r * E + e, load4<T>(dout + (n * (k + 1) + 1 + j) * E + e));
    }
}

// dpos[0] (and dcls) = sum_f dout[f][0] ; dpos[1 + p] = sum over the frames that kept p of dout[f][1 + slot[f, p]]. One thread per 4
// columns of one position walks the frames in order with four independent partial sums (frame f goes to sum f % 4, the last N % 4
// frames to sum 0): a fixed order, fp32 accumulation, one rounding at the store. acc: += (the destinations are gradient-arena slots).
template <typename T>
__global__ void assemble_kept_bwd_pos_kernel(const T* dout, const int32_t* __restrict__ slot, T* dpos, T* dcls, int N, int Pn, int k, int E, int acc) {
    const int E4 = E / 4;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)(Pn + 1) * E4) return;
    const int e = (int)(q % E4) * 4, t = (int)(q / E4);
    const int64_t fs = (int64_t)(k + 1) * E;
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    f32x4_t s0 = zero, s1 = zero, s2 = zero, s3 = zero;
    if (t == 0) {
        int n = 0;
        for (; n + 4 <= N; n += 4) {
            const f32x4_t a0 = load4<T>(dout + (n + 0) * fs + e), a1 = load4<T>(dout + (n + 1) * fs + e);
            const f32x4_t a2 = load4<T>(dout + (n + 2) * fs + e), a3 = load4<T>(dout + (n + 3) * fs + e);
            s0 += a0; s1 += a1; s2 += a2; s3 += a3;
        }
        for (; n < N; ++n) s0 += load4<T>(dout + n * fs + e);
    } else {
        const int32_t* sp = slot + (t - 1);
        int n = 0;
        for (; n + 4 <= N; n += 4) {
            const int j0 = sp[(int64_t)(n + 0) * Pn], j1 = sp[(int64_t)(n + 1) * Pn], j2 = sp[(int64_t)(n + 2) * Pn], j3 = sp[(int64_t)(n + 3) * Pn];
            const bool k0 = j0 >= 0 && j0 < k, k1 = j1 >= 0 && j1 < k, k2 = j2 >= 0 && j2 < k, k3 = j3 >= 0 && j3 < k;
            const f32x4_t a0 = k0 ? load4<T>(dout + (n + 0) * fs + (int64_t)(1 + j0) * E + e) : zero;
            const f32x4_t a1 = k1 ? load4<T>(dout + (n + 1) * fs + (int64_t)(1 + j1) * E + e) : zero;
            const f32x4_t a2 = k2 ? load4<T>(dout + (n + 2) * fs + (int64_t)(1 + j2) * E + e) : zero;
            const f32x4_t a3 = k3 ? load4<T>(dout + (n + 3) * fs + (int64_t)(1 + j3) * E + e) : zero;
            s0 += a0; s1 += a1; s2 += a2; s3 += a3;
        }
        for (; n < N; ++n) {
            const int sn = sp[(int64_t)n * Pn];
            if (sn >= 0 && sn < k) s0 += load4<T>(dout + n * fs + (int64_t)(1 + sn) * E + e);
        }
    }
    const f32x4_t sum = (s0 + s1) + (s2 + s3);
    T* d = dpos + (int64_t)t * E + e;
    store4<T>(d, acc ? sum + load4<T>(d) : sum);
    if (dcls && t == 0) store4<T>(dcls + e, acc ? sum + load4<T>(dcls + e) : sum);
}

static inline int grid_for(int64_t work, int block = 256, int cap = 8192) {
    int64_t g = (work + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}
#define DISPATCH_T(dtype, CALL_BF16, CALL_F32)              \
    if ((dtype) == VALOR_DT_BF16) { CALL_BF16; }            \
    else if ((dtype) == VALOR_DT_F32) { CALL_F32; }         \
    else return VALOR_ERR_ARG;

extern "C" int valor_patch_keep(void* stream, int N, int Pn, int k, int group, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                                int32_t* idx, int32_t* slot) {
    if (!idx || !slot) return VALOR_ERR_ARG;
    if (N <= 0 || Pn < 1 || Pn > KEEP_MAX_PN || k < 1 || k > Pn || group < 1 || N % group) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(patch_keep_kernel, dim3(N / group), dim3(WAVE), 0, (hipStream_t)stream, Pn, k, group, seed, offset, rng_base, idx, slot);
    return valor_launch_status();
}

extern "C" int valor_patchify_kept(void* stream, int dtype, const float* in, const int32_t* idx, void* out, int N, int C, int H, int W, int P,
                                   int k, int64_t ld_out) {
    if (N <= 0) return VALOR_OK;
    const int64_t K = (int64_t)C * P * P;
    if (ld_out <= 0) ld_out = K;
    if (!in || !idx || !out || C <= 0 || P <= 0 || (P & 1) || H <= 0 || W <= 0 || H % P || W % P || ld_out < K) return VALOR_ERR_ARG;
    if (k < 1 || (int64_t)k > (int64_t)(H / P) * (W / P)) return VALOR_ERR_ARG;
    const bool v4 = (P & 3) == 0 && (ld_out & 3) == 0;
    if (!v4 && (W & 1)) return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t work = (int64_t)N * k * K / (v4 ? 4 : 2);
    if (v4) {
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((patchify_kept_kernel<bf16_t, 4>), dim3(grid_for(work)), dim3(256), 0, st, in, idx, (bf16_t*)out, N, C, H, W, P, k, ld_out),
            hipLaunchKernelGGL((patchify_kept_kernel<float, 4>), dim3(grid_for(work)), dim3(256), 0, st, in, idx, (float*)out, N, C, H, W, P, k, ld_out));
    } else {
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((patchify_kept_kernel<bf16_t, 2>), dim3(grid_for(work)), dim3(256), 0, st, in, idx, (bf16_t*)out, N, C, H, W, P, k, ld_out),
            hipLaunchKernelGGL((patchify_kept_kernel<float, 2>), dim3(grid_for(work)), dim3(256), 0, st, in, idx, (float*)out, N, C, H, W, P, k, ld_out));
    }
    return valor_launch_status();
}

extern "C" int valor_assemble_tokens_kept_fwd(void* stream, int dtype, const void* patches, const void* cls, const void* pos, const void* bias,
                                              const int32_t* idx, void* out, int N, int Pn, int k, int E) {
    if (N <= 0) return VALOR_OK;
    if (!patches || !cls || !pos || !idx || !out || Pn < 1 || k < 1 || k > Pn || E <= 0 || (E & 3)) return VALOR_ERR_ARG;   // bias is optional
    hipStream_t st = (hipStream_t)stream;
    const int64_t work = (int64_t)N * (k + 1) * E / 4;
    DISPATCH_T(dtype,
        hipLaunchKernelGGL((assemble_kept_fwd_kernel<bf16_t>), dim3(grid_for(work)), dim3(256), 0, st, (const bf16_t*)patches, (const bf16_t*)cls, (const bf16_t*)pos, (const bf16_t*)bias, idx, (bf16_t*)out, N, Pn, k, E),
        hipLaunchKernelGGL((assemble_kept_fwd_kernel<float>), dim3(grid_for(work)), dim3(256), 0, st, (const float*)patches, (const float*)cls, (const float*)pos, (const float*)bias, idx, (float*)out, N, Pn, k, E));
    return valor_launch_status();
}

extern "C" int valor_assemble_tokens_kept_bwd(void* stream, int dtype, const void* dout, const int32_t* slot, void* dpatches, void* dpos, void* dcls,
                                              int N, int Pn, int k, int E, int accumulate) {
    if (N <= 0) return VALOR_OK;
    if (!dout || !slot || !dpatches || !dpos || Pn < 1 || k < 1 || k > Pn || E <= 0 || (E & 3)) return VALOR_ERR_ARG;       // dcls is optional
    hipStream_t st = (hipStream_t)stream;
    const int64_t work = (int64_t)N * k * E / 4, work2 = (int64_t)(Pn + 1) * E / 4;
    DISPATCH_T(dtype,
        { hipLaunchKernelGGL((assemble_kept_bwd_patches_kernel<bf16_t>), dim3(grid_for(work)), dim3(256), 0, st, (const bf16_t*)dout, (bf16_t*)dpatches, N, k, E);
          hipLaunchKernelGGL((assemble_kept_bwd_pos_kernel<bf16_t>), dim3(grid_for(work2, 256, 1 << 20)), dim3(256), 0, st, (const bf16_t*)dout, slot, (bf16_t*)dpos, (bf16_t*)dcls, N, Pn, k, E, accumulate); },
        { hipLaunchKernelGGL((assemble_kept_bwd_patches_kernel<float>), dim3(grid_for(work)), dim3(256), 0, st, (const float*)dout, (float*)dpatches, N, k, E);
          hipLaunchKernelGGL((assemble_kept_bwd_pos_kernel<float>), dim3(grid_for(work2, 256, 1 << 20)), dim3(256), 0, st, (const float*)dout, slot, (float*)dpos, (float*)dcls, N, Pn, k, E, accumulate); });
    return valor_launch_status();
}
