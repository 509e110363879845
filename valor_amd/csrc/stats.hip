// Training diagnostics over the flat arenas: per-tensor and per-group statistics of the gradients (between the clip and the update, which
// clears them) and of the weights / the Adam term (behind the update). Nothing is read back, nothing that is trained is written.
//
// A row is 8 floats. valor_arena_grad_stats owns fields 0-3, valor_arena_update_stats fields 4-7:
//   0 g_sumsq      sum of g^2 over the tensor's FINITE elements, unscaled          4 w_sumsq   sum of w^2 (fp32 master)
//   1 g_absmax     max |g| over the finite elements                                5 u_sumsq   sum of u^2, u = lr_g * bc[1] / bc[0] * m / (sqrtf(v) + eps)
//   2 g_nonfinite  number of inf / NaN elements (fp32 counter)                     6 w_norm    sqrt(w_sumsq)
//   3 g_norm       sqrt(g_sumsq) * norm_mul (the units of total_norm)              7 u_ratio   sqrt(u_sumsq) / (w_norm + 1e-12)
// u is the Adam term adamw_kernel (optim.hip) has just applied, from the moments as they stand behind the step; the decay term is not part
// of it. A non-finite *gscale (the step was skipped, the moments are the old ones) makes fields 5 and 7 zero in every row. An inactive
// tensor (chunk_group < 0 on its chunks) has zeros in the fields of the call; a group row is the fold of its active tensors: sums and
// maxima of the tensor rows, norms and ratios recomputed from the folded sums.
//
// Layout: tensor t occupies ceil(tensor_numel[t] / chunk) consecutive chunks (ParamArena); only its tensor_numel[t] elements count, the
// padding behind its tail is loaded with the rest of the chunk and dropped by a select, never by a multiplication (it may hold NaN).
//
// Three launches per call, no floating-point atomics, every reduction of a fixed shape:
//   1. *_partial_kernel: ONE streaming read of the arena(s). A wave owns a chunk: 16-byte loads, 1 KiB per wave-instruction, eight (grad)
//      or twelve (update: three arenas) of them in flight per lane. The loads are unconditional -- the chunk tables are read while they fly and
//      only select afterwards (optim.hip, sumsq_kernel, records what a load that waits for the group byte costs). Per chunk: a lane sums
//      its 4 .. 16 elements in order, a butterfly over the 64 lanes, lane 0 stores the chunk's partial. The first chunk of a tensor also
//      records itself in first[t]. The gradient pass tries a full, finite chunk without the per-element tests first (same terms, same order).
//   2. tensor_reduce_kernel: a block per tensor; thread i adds the partials of the chunks i, i + 256, ... in chunk order, in fp64, then
//      a butterfly and the four waves in order. A tensor's row depends on its own chunks alone.
//   3. group_fold_kernel: thread g walks the tensor rows in tensor-index order and adds those of group g in fp64.
// Error of a sum of squares against exact arithmetic: the fp32 part is the chunk partial (<= 16 sequential fused multiply-adds and six
// butterfly levels: below 23 ulp, 1.4e-6 relative for non-negative terms); the fp64 stages add one fp32 rounding each when the tensor row
// and the group row are stored. Well inside the 1e-5 the tests ask for, independent of the tensor's size.
#include "common.h"

#define STATS_CHUNK 1024
#define STATS_MAX_GROUPS 16
#define STATS_FIELDS 8
#define STATS_FOLD_TILE 1024

struct StatsLr {
    float lr[STATS_MAX_GROUPS];
};

DEVINL double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the number of chunk c's elements that belong to its tensor (0: none), from the (wave-uniform) tables; the first chunk of a tensor also
// leaves the entry first[t]. The tables are __restrict__ and their addresses wave-uniform: the compiler reads them with scalar loads, which have a counter of their
// own and do not queue behind the arena loads. The group byte has no scalar load on gfx950: the kernels read it in FRONT of the arena
// loads, so waiting for it leaves those in flight.
DEVINL int chunk_valid(const int32_t* __restrict__ chunk_tensor, const int64_t* __restrict__ tensor_numel, int ntensors, int64_t nchunks,
                       int64_t c, int lane, int32_t* __restrict__ first) {
    const int t = chunk_tensor[c];
    const int tn = c + 1 < nchunks ? chunk_tensor[c + 1] : -1;
    const int tp = c > 0 ? chunk_tensor[c - 1] : -1;
    int valid = 0;
    if (t >= 0 && t < ntensors) {
        const int64_t ne = tensor_numel[t];
        if (ne > 0) valid = tn == t ? STATS_CHUNK : (int)((ne - 1) % STATS_CHUNK) + 1;
        if (tp != t && lane == 0) first[t] = (int32_t)c;
    }
    return valid;
}

struct GradAcc {
    float s, mx, nf;
};
DEVINL void grad_acc(GradAcc& a, uint32_t bits, bool in) {
    const bool fin = (bits & 0x7f800000u) != 0x7f800000u;
    const float x = (in && fin) ? fabsf(__uint_as_float(bits)) : 0.f;
    a.s = fmaf(x, x, a.s);
    a.mx = fmaxf(a.mx, x);
    a.nf += (in && !fin) ? 1.f : 0.f;
}

// partial[c] = (sum of squares, max |g|, non-finite count, 0) of chunk c's elements inside its tensor; zeros for an inactive chunk
template <typename T>
__global__ __launch_bounds__(256) void grad_partial_kernel(const T* __restrict__ grad, const int8_t* __restrict__ chunk_group,
                                                           const int32_t* __restrict__ chunk_tensor, const int64_t* __restrict__ tensor_numel,
                                                           int ntensors, int64_t nchunks, int32_t* __restrict__ first,
                                                           f32x4_t* __restrict__ partial) {
    constexpr int L = sizeof(T) == 2 ? 2 : 4;          // 16-byte loads per lane and chunk: a wave covers 1 KiB per load
    constexpr int U = 8 / L;                           // chunks in flight per wave
    constexpr int E = 16 / (int)sizeof(T);             // elements per load and lane
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t c0 = wave; c0 < nchunks; c0 += nw * U) {
        u32x4_t r[U][L];
        int valid_of[U], gid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c = c0 + u * nw;
            gid[u] = chunk_group[c < nchunks ? c : nchunks - 1];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c = c0 + u * nw;
            const int64_t cl = c < nchunks ? c : nchunks - 1;
            const char* base = (const char*)grad + cl * (int64_t)(STATS_CHUNK * sizeof(T)) + lane * 16;
#pragma unroll
            for (int j = 0; j < L; ++j) r[u][j] = *(const u32x4_t*)(base + j * 1024);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c = c0 + u * nw;
            valid_of[u] = c < nchunks ? chunk_valid(chunk_tensor, tensor_numel, ntensors, nchunks, c, lane, first) : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c = c0 + u * nw;
            if (c >= nchunks) continue;
            GradAcc a = {0.f, 0.f, 0.f};
            const int valid = valid_of[u];
            // The common chunk is full and finite, and then needs neither the bounds nor the finite test: sum and maximum of everything
            // that was loaded. The sum says whether that was right -- an inf or NaN anywhere makes it non-finite -- and it is the same
            // in every lane behind the butterfly. The general pass below adds the same terms in the same order, so which pass served
            // a chunk does not show in the bits. (With both tests on every element the kernel was bound by VALU issue: 815 vector
            // instructions per wave for 8 KB, as long as the SIMD's share of the HBM stream takes; 3.6 TB/s.)
#pragma unroll
            for (int j = 0; j < L; ++j) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if constexpr (sizeof(T) == 2) {
                        const float lo = __uint_as_float(r[u][j][k] << 16), hi = __uint_as_float(r[u][j][k] & 0xffff0000u);
                        a.s = fmaf(lo, lo, a.s);
                        a.mx = fmaxf(a.mx, fabsf(lo));
                        a.s = fmaf(hi, hi, a.s);
                        a.mx = fmaxf(a.mx, fabsf(hi));
                    } else {
                        const float x = __uint_as_float(r[u][j][k]);
                        a.s = fmaf(x, x, a.s);
                        a.mx = fmaxf(a.mx, fabsf(x));
                    }
                }
            }
            a.s = wave_sum(a.s);
            const bool plain = valid == STATS_CHUNK && (__builtin_amdgcn_readfirstlane(__float_as_uint(a.s)) & 0x7f800000u) != 0x7f800000u;
            if (!plain) {
                a = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < L; ++j) {
                    const int e0 = j * (64 * E) + lane * E;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if constexpr (sizeof(T) == 2) {
                            grad_acc(a, r[u][j][k] << 16, e0 + 2 * k < valid);
                            grad_acc(a, r[u][j][k] & 0xffff0000u, e0 + 2 * k + 1 < valid);
                        } else {
                            grad_acc(a, r[u][j][k], e0 + k < valid);
                        }
                    }
                }
                a.s = wave_sum(a.s);
                a.nf = wave_sum(a.nf);
            }
            a.mx = wave_max(a.mx);
            if (lane == 0) partial[c] = gid[u] >= 0 ? (f32x4_t){a.s, a.mx, a.nf, 0.f} : (f32x4_t){0.f, 0.f, 0.f, 0.f};
        }
    }
}

// partial[c] = (sum of w^2, sum of u^2, 0, 0) of chunk c's elements inside its tensor; zeros for an inactive chunk
__global__ __launch_bounds__(256) void update_partial_kernel(const float* __restrict__ master, const float* __restrict__ exp_avg,
                                                             const float* __restrict__ exp_avg_sq, const int8_t* __restrict__ chunk_group,
                                                             const int32_t* __restrict__ chunk_tensor, const f32x2_t* __restrict__ chunk_bc,
                                                             const int64_t* __restrict__ tensor_numel, int ntensors, int64_t nchunks,
                                                             StatsLr groups, float eps, int32_t* __restrict__ first,
                                                             f32x4_t* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t c = wave; c < nchunks; c += nw) {
        f32x4_t w[4], m[4], v[4];
        const int gid = chunk_group[c];
        const int64_t off = c * STATS_CHUNK + lane * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[j] = *(const f32x4_t*)(master + off + j * 256);
            m[j] = *(const f32x4_t*)(exp_avg + off + j * 256);
            v[j] = *(const f32x4_t*)(exp_avg_sq + off + j * 256);
        }
        const int valid = chunk_valid(chunk_tensor, tensor_numel, ntensors, nchunks, c, lane, first);
        const bool on = gid >= 0 && gid < STATS_MAX_GROUPS;
        const f32x2_t bc = chunk_bc[c];
        const float step_size = (on ? groups.lr[gid] : 0.f) * bc[1] / bc[0];       // adamw_kernel's step_size, same roundings
        float ws = 0.f, us = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = j * 256 + lane * 4 + k < valid;
                const float wk = in ? w[j][k] : 0.f;
                const float uk = in ? step_size * (m[j][k] / (sqrtf(v[j][k]) + eps)) : 0.f;
                ws = fmaf(wk, wk, ws);
                us = fmaf(uk, uk, us);
            }
        }
        ws = wave_sum(ws);
        us = wave_sum(us);
        if (lane == 0) partial[c] = on ? (f32x4_t){ws, us, 0.f, 0.f} : (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
}

// MODE 0: fields 0-3 of tensor t from the grad partials; MODE 1: fields 4-7 from the update partials. tgroup[t] = the tensor's group, -1 if
// it is inactive (or has no chunk). first[t] is trusted only if the chunk it names IS the first chunk of t: an entry nobody wrote this call
// (a tensor without a chunk) cannot pass for one.
template <int MODE>
__global__ __launch_bounds__(256) void tensor_reduce_kernel(const f32x4_t* partial, const int32_t* first, int32_t* tgroup,
                                                            const int8_t* chunk_group, const int32_t* chunk_tensor, const int64_t* tensor_numel,
                                                            int64_t nchunks, int ngroups, float norm_mul, const float* gscale_dev,
                                                            f32x4_t* tensor_stats) {
    __shared__ double red_a[4], red_b[4];
    __shared__ float red_m[4];
    const int t = blockIdx.x;
    const int64_t f = first[t], ne = tensor_numel[t];
    bool ok = ne > 0 && f >= 0 && f < nchunks;
    if (ok) ok = chunk_tensor[f] == t && (f == 0 || chunk_tensor[f - 1] != t);
    int g = ok ? (int)chunk_group[f] : -1;
    if (g >= ngroups) g = -1;
    int64_t nc = ok ? (ne + STATS_CHUNK - 1) / STATS_CHUNK : 0;
    if (ok && f + nc > nchunks) nc = nchunks - f;
    double a = 0.0, b = 0.0;
    float mx = 0.f;
    if (g >= 0) {
        // sixteen partials in flight per thread (the word embeddings are 22.9k chunks: ninety dependent round trips one at a time); a
        // slot behind the tensor's end adds zeros, which leave the non-negative sums and the maximum as they are
        constexpr int R = 16;
        for (int64_t c = threadIdx.x; c < nc; c += 256 * R) {
            f32x4_t p[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t cr = c + r * 256;
                p[r] = cr < nc ? partial[f + cr] : (f32x4_t){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a += (double)p[r][0];
                if (MODE == 0) { mx = fmaxf(mx, p[r][1]); b += (double)p[r][2]; }
                else b += (double)p[r][1];
            }
        }
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { red_a[threadIdx.x >> 6] = a; red_b[threadIdx.x >> 6] = b; red_m[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((red_a[0] + red_a[1]) + red_a[2]) + red_a[3];
        b = ((red_b[0] + red_b[1]) + red_b[2]) + red_b[3];
        mx = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        f32x4_t row;
        if (MODE == 0) {
            const float s = (float)a;
            row = (f32x4_t){s, mx, (float)b, sqrtf(s) * norm_mul};
        } else {
            const bool skip = gscale_dev && !(fabsf(*gscale_dev) < INFINITY);
            const float ws = (float)a, us = skip ? 0.f : (float)b, wn = sqrtf(ws);
            row = (f32x4_t){ws, us, wn, sqrtf(us) / (wn + 1e-12f)};
        }
        tensor_stats[(int64_t)t * 2 + MODE] = row;
        tgroup[t] = g;
    }
}

// thread g < ngroups folds the tensor rows of group g in tensor-index order (fp64 sums); the rows pass through LDS a tile at a time
template <int MODE>
__global__ __launch_bounds__(256) void group_fold_kernel(const f32x4_t* tensor_stats, const int32_t* tgroup, int ntensors, int ngroups,
                                                         float norm_mul, f32x4_t* group_stats) {
    __shared__ f32x4_t rows[STATS_FOLD_TILE];
    __shared__ int gid[STATS_FOLD_TILE];
    double a = 0.0, b = 0.0;
    float mx = 0.f;
    for (int base = 0; base < ntensors; base += STATS_FOLD_TILE) {
        for (int i = threadIdx.x; i < STATS_FOLD_TILE; i += 256) {
            const int t = base + i;
            if (t < ntensors) { rows[i] = tensor_stats[(int64_t)t * 2 + MODE]; gid[i] = tgroup[t]; }
            else gid[i] = -1;
        }
        __syncthreads();
        if ((int)threadIdx.x < ngroups) {
            const int m = ntensors - base < STATS_FOLD_TILE ? ntensors - base : STATS_FOLD_TILE;
            // branch-free, so the LDS reads run ahead of the additions: a row of another group adds zeros (the sums are non-negative: no bit moves)
#pragma unroll 8
            for (int i = 0; i < m; ++i) {
                const bool mine = gid[i] == (int)threadIdx.x;
                const f32x4_t p = rows[i];
                a += mine ? (double)p[0] : 0.0;
                if (MODE == 0) { mx = fmaxf(mx, mine ? p[1] : 0.f); b += mine ? (double)p[2] : 0.0; }
                else b += mine ? (double)p[1] : 0.0;
            }
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < ngroups) {
        f32x4_t row;
        if (MODE == 0) {
            const float s = (float)a;
            row = (f32x4_t){s, mx, (float)b, sqrtf(s) * norm_mul};
        } else {
            const float ws = (float)a, us = (float)b, wn = sqrtf(ws);
            row = (f32x4_t){ws, us, wn, sqrtf(us) / (wn + 1e-12f)};
        }
        group_stats[threadIdx.x * 2 + MODE] = row;
    }
}

// scratch (fp32 words, 16-byte aligned): first[ntensors rounded up to 4] | tgroup[the same] | partial[4 * nchunks]
struct StatsScratch {
    int32_t* first;
    int32_t* tgroup;
    f32x4_t* partial;
};
static StatsScratch stats_scratch(float* scratch, int ntensors) {
    const int64_t nt4 = ((int64_t)ntensors + 3) / 4 * 4;
    StatsScratch s;
    s.first = (int32_t*)scratch;
    s.tgroup = s.first + nt4;
    s.partial = (f32x4_t*)(scratch + 2 * nt4);
    return s;
}
static bool stats_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
// at most 1024 blocks (four per CU, as sumsq_kernel): all of them are resident at once and take equal shares of the chunks. 2048 did not
// fit (five to seven waves per SIMD): the blocks left over ran as a second, nearly empty round and the gradient pass read at 3.7 TB/s.
static int stats_blocks(int64_t nchunks, int per_wave) {
    const int64_t b = (nchunks + 4 * per_wave - 1) / (4 * per_wave);
    return (int)(b < 1024 ? b : 1024);
}

extern "C" int valor_arena_grad_stats(void* stream, int dtype, const void* grad, const int8_t* chunk_group, const int32_t* chunk_tensor,
                                      const int64_t* tensor_numel, int ntensors, int64_t n, int ngroups, float norm_mul, float* scratch,
                                      float* tensor_stats, float* group_stats) {
    if (n == 0) return VALOR_OK;
    if (n < 0 || (n % STATS_CHUNK) || valor_adamw_chunk() != STATS_CHUNK || ntensors < 1 || ngroups < 1 || ngroups > STATS_MAX_GROUPS
        || !grad || !chunk_group || !chunk_tensor || !tensor_numel || !scratch || !tensor_stats || !group_stats)
        return VALOR_ERR_ARG;
    if (dtype != VALOR_DT_BF16 && dtype != VALOR_DT_F32) return VALOR_ERR_ARG;
    if (stats_misaligned(grad, 16) || stats_misaligned(scratch, 16) || stats_misaligned(tensor_stats, 16) || stats_misaligned(group_stats, 16)
        || stats_misaligned(chunk_tensor, 4) || stats_misaligned(tensor_numel, 8))
        return VALOR_ERR_ARG;
    const int64_t nchunks = n / STATS_CHUNK;
    const StatsScratch s = stats_scratch(scratch, ntensors);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VALOR_DT_BF16)
        hipLaunchKernelGGL((grad_partial_kernel<bf16_t>), dim3(stats_blocks(nchunks, 4)), dim3(256), 0, st, (const bf16_t*)grad, chunk_group,
                           chunk_tensor, tensor_numel, ntensors, nchunks, s.first, s.partial);
    else
        hipLaunchKernelGGL((grad_partial_kernel<float>), dim3(stats_blocks(nchunks, 2)), dim3(256), 0, st, (const float*)grad, chunk_group,
                           chunk_tensor, tensor_numel, ntensors, nchunks, s.first, s.partial);
    int rc = valor_launch_status();
    if (rc != VALOR_OK) return rc;
    hipLaunchKernelGGL((tensor_reduce_kernel<0>), dim3(ntensors), dim3(256), 0, st, s.partial, s.first, s.tgroup, chunk_group, chunk_tensor,
                       tensor_numel, nchunks, ngroups, norm_mul, (const float*)nullptr, (f32x4_t*)tensor_stats);
    rc = valor_launch_status();
    if (rc != VALOR_OK) return rc;
    hipLaunchKernelGGL((group_fold_kernel<0>), dim3(1), dim3(256), 0, st, (const f32x4_t*)tensor_stats, s.tgroup, ntensors, ngroups, norm_mul,
                       (f32x4_t*)group_stats);
    return valor_launch_status();
}

extern "C" int valor_arena_update_stats(void* stream, const float* master, const float* exp_avg, const float* exp_avg_sq,
                                        const int8_t* chunk_group, const int32_t* chunk_tensor, const float* chunk_bc,
                                        const int64_t* tensor_numel, int ntensors, int64_t n, const float* lr, int ngroups, float eps,
                                        const float* gscale_dev, float* scratch, float* tensor_stats, float* group_stats) {
    if (n == 0) return VALOR_OK;
    if (n < 0 || (n % STATS_CHUNK) || valor_adamw_chunk() != STATS_CHUNK || ntensors < 1 || ngroups < 1 || ngroups > STATS_MAX_GROUPS
        || !master || !exp_avg || !exp_avg_sq || !chunk_group || !chunk_tensor || !chunk_bc || !tensor_numel || !lr || !scratch
        || !tensor_stats || !group_stats)
        return VALOR_ERR_ARG;
    if (stats_misaligned(master, 16) || stats_misaligned(exp_avg, 16) || stats_misaligned(exp_avg_sq, 16) || stats_misaligned(scratch, 16)
        || stats_misaligned(tensor_stats, 16) || stats_misaligned(group_stats, 16) || stats_misaligned(chunk_tensor, 4)
        || stats_misaligned(chunk_bc, 8) || stats_misaligned(tensor_numel, 8) || stats_misaligned(gscale_dev, 4))
        return VALOR_ERR_ARG;
    const int64_t nchunks = n / STATS_CHUNK;
    const StatsScratch s = stats_scratch(scratch, ntensors);
    StatsLr g;
    for (int i = 0; i < STATS_MAX_GROUPS; ++i) g.lr[i] = i < ngroups ? lr[i] : 0.f;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(update_partial_kernel, dim3(stats_blocks(nchunks, 1)), dim3(256), 0, st, master, exp_avg, exp_avg_sq, chunk_group,
                       chunk_tensor, (const f32x2_t*)chunk_bc, tensor_numel, ntensors, nchunks, g, eps, s.first, s.partial);
    int rc = valor_launch_status();
    if (rc != VALOR_OK) return rc;
    hipLaunchKernelGGL((tensor_reduce_kernel<1>), dim3(ntensors), dim3(256), 0, st, s.partial, s.first, s.tgroup, chunk_group, chunk_tensor,
                       tensor_numel, nchunks, ngroups, 1.0f, gscale_dev, (f32x4_t*)tensor_stats);
    rc = valor_launch_status();
    if (rc != VALOR_OK) return rc;
    hipLaunchKernelGGL((group_fold_kernel<1>), dim3(1), dim3(256), 0, st, (const f32x4_t*)tensor_stats, s.tgroup, ntensors, ngroups, 1.0f,
                       (f32x4_t*)group_stats);
    return valor_launch_status();
}
