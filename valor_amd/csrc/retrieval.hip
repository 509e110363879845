// Retrieval evaluation: the rank of every query's ground truth in a score matrix, WITHOUT a sort (test.py:685-775 compute_dualsoftmax_*
// and compute_metric_ret). The rank of a ground truth is the number of candidates that beat it, so one streaming read of the matrix
// with a compare per element replaces sort + tolist + list.index. See include/valor_hip.h for the contract and the tie rule.
//
// Tiling (every pass): a workgroup of four waves owns RT_ROWS = 32 consecutive rows and walks ALL columns; wave w takes the column
// chunks c = w, w + 4, ... of 256 columns (64 lanes x 4 columns), eight rows in flight per lane. Row quantities (log-sum-exp of a row,
// forward count of a text) stay in lane-private registers across the chunks and are reduced once per workgroup (shuffles, then LDS
// across the four waves). Column quantities (log-sum-exp of a column, backward count of a clip) are complete over the 32 rows at the end
// of a chunk and go to a [row blocks, Nv] partial buffer that one small kernel reduces: no float atomics, no [Nt, Nv] temporary.
// Lanes run along j (coalesced 16-byte loads where ld % 4 == 0 and the base is 16-byte aligned, four 4-byte loads 64 columns apart
// otherwise), the loop runs over i.
//
// Passes over the matrix: 1 without dual softmax (the rank pass; both directions share it), 2 with it (the statistics pass producing
// both log-sum-exp vectors, then the rank pass). In between one thread per text / clip evaluates the ground-truth thresholds with the SAME
// device function the rank pass uses, so a ground truth always compares equal to itself.
#include "common.h"
#include <math.h>

#define RT_ROWS 32
#define RT_WAVES 4
#define RT_COLS 256
#define RT_LOG2E 1.44269504088896340736f
#define RT_LN2 0.69314718055994530942f

// score * softmax * n (test.py:694 / :710): s * exp(s / temp - lse) * n. Everything between the score and the exponential is kept in
// base 2 (k2 = log2(e) / temp, lse2 = log2 of the sum): ONE rounding, that of the fused multiply-add, in front of v_exp_f32.
DEVINL float ret_dual_val(float s, float k2, float lse2, float n) { return s * hw_exp2(fmaf(s, k2, -lse2)) * n; }
DEVINL float ret_exp(float x) { return hw_exp2(x); }

// the four values of row `row` this lane owns in the chunk starting at column j0; NaN outside the matrix
template <bool VEC4> DEVINL void ret_load4(const float* score, int64_t ld, int row, int Nt, int j0, int lane, int Nv, float* v) {
    const float nanv = __uint_as_float(0x7fc00000u);
    if (row >= Nt) {
        v[0] = v[1] = v[2] = v[3] = nanv;
        return;
    }
    const float* p = score + (int64_t)row * ld;
    if constexpr (VEC4) {
        const int j = j0 + 4 * lane;
        if (j < Nv) {                       // ld % 4 == 0 and j % 4 == 0: j + 3 < ld, the load stays inside the row
            const f32x4_t t = *(const f32x4_t*)(p + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (j + e < Nv) ? t[e] : nanv;
        } else {
            v[0] = v[1] = v[2] = v[3] = nanv;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + lane + 64 * e;
            v[e] = (j < Nv) ? p[j] : nanv;
        }
    }
}
template <bool VEC4> DEVINL int ret_col(int j0, int lane, int e) { return VEC4 ? j0 + 4 * lane + e : j0 + lane + 64 * e; }

// online (max, sum) update with n new values
template <int N> DEVINL void ret_online(float& m, float& s, const float* v) {
    float mx = v[0];
#pragma unroll
    for (int r = 1; r < N; ++r) mx = fmaxf(mx, v[r]);
    const float nm = fmaxf(m, mx);
    const float ref = (nm == -INFINITY) ? 0.f : nm;       // nothing seen yet: exp(-inf - 0) = 0 instead of exp(-inf + inf)
    float acc = s * ret_exp(m - ref);
#pragma unroll
    for (int r = 0; r < N; ++r) acc += ret_exp(v[r] - ref);
    m = nm;
    s = acc;
}
DEVINL void ret_merge(float& m, float& s, float m2, float s2) {
    const float nm = fmaxf(m, m2);
    const float ref = (nm == -INFINITY) ? 0.f : nm;
    s = s * ret_exp(m - ref) + s2 * ret_exp(m2 - ref);
    m = nm;
}

// ---------------------------------------------------------------- pass 1 (dual softmax only): lse_row, column partials
template <bool VEC4>
__global__ __launch_bounds__(256) void ret_stats_kernel(const float* __restrict__ score, int64_t ld, float k, float* __restrict__ lse_row,
                                                        float* __restrict__ lse2_row, float* __restrict__ part_m,
                                                        float* __restrict__ part_s, int Nt, int Nv) {
    __shared__ float sh_m[RT_WAVES][RT_ROWS], sh_s[RT_WAVES][RT_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * RT_ROWS;
    float rm[RT_ROWS], rs[RT_ROWS];
#pragma unroll
    for (int r = 0; r < RT_ROWS; ++r) { rm[r] = -INFINITY; rs[r] = 0.f; }
    const int nchunk = (Nv + RT_COLS - 1) / RT_COLS;
    for (int c = wave; c < nchunk; c += RT_WAVES) {
        const int j0 = c * RT_COLS;
        float cm[4], cs[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { cm[e] = -INFINITY; cs[e] = 0.f; }
#pragma unroll
        for (int rg = 0; rg < RT_ROWS / 8; ++rg) {
            float v[8][4];
#pragma unroll
            for (int r = 0; r < 8; ++r) ret_load4<VEC4>(score, ld, i0 + rg * 8 + r, Nt, j0, lane, Nv, v[r]);
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = (i0 + rg * 8 + r < Nt) && (ret_col<VEC4>(j0, lane, e) < Nv);
                    v[r][e] = in ? v[r][e] * k : -INFINITY;          // a NaN score stays NaN: its row and column get a NaN lse
                }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float col[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) col[r] = v[r][e];
                ret_online<8>(cm[e], cs[e], col);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) ret_online<4>(rm[rg * 8 + r], rs[rg * 8 + r], v[r]);
            __builtin_amdgcn_sched_barrier(0);          // eight rows in flight, not thirty-two: keeps the loads of the next group below this point
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = ret_col<VEC4>(j0, lane, e);
            if (j < Nv) {
                part_m[(int64_t)blockIdx.x * Nv + j] = cm[e];
                part_s[(int64_t)blockIdx.x * Nv + j] = cs[e];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RT_ROWS; ++r) {
        float m = rm[r], s = rs[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
            ret_merge(m, s, m2, s2);
        }
        if (lane == 0) { sh_m[wave][r] = m; sh_s[wave][r] = s; }
    }
    __syncthreads();
    if (threadIdx.x < RT_ROWS && i0 + (int)threadIdx.x < Nt) {
        float m = sh_m[0][threadIdx.x], s = sh_s[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < RT_WAVES; ++w) ret_merge(m, s, sh_m[w][threadIdx.x], sh_s[w][threadIdx.x]);
        const float l2 = m + __log2f(s);
        lse2_row[i0 + threadIdx.x] = l2;
        if (lse_row) lse_row[i0 + threadIdx.x] = l2 * RT_LN2;
    }
}

__global__ __launch_bounds__(256) void ret_stats_finalize_kernel(const float* __restrict__ part_m, const float* __restrict__ part_s,
                                                                 float* __restrict__ lse_col, float* __restrict__ lse2_col, int nblk,
                                                                 int Nv) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Nv) return;
    float m = -INFINITY, s = 0.f;
    for (int b = 0; b < nblk; ++b) ret_merge(m, s, part_m[(int64_t)b * Nv + j], part_s[(int64_t)b * Nv + j]);
    const float l2 = m + __log2f(s);
    lse2_col[j] = l2;
    if (lse_col) lse_col[j] = l2 * RT_LN2;
}

// ---------------------------------------------------------------- thresholds: one thread per text and per clip
// xg[i] = x[i, gt_col[i]] (NaN for a gt_col outside [0, Nv)); per clip the best ground-truth text (col_m, col_i; col_i = -1: none)
template <bool DUAL>
__global__ __launch_bounds__(256) void ret_thresh_kernel(const float* __restrict__ score, int64_t ld, const int* __restrict__ gt_col,
                                                         const int* __restrict__ col_ptr, const int* __restrict__ col_rows, int nnz, float k,
                                                         const float* __restrict__ lse_row, const float* __restrict__ lse_col,
                                                         float* __restrict__ xg, float* __restrict__ col_m, int* __restrict__ col_i,
                                                         int Nt, int Nv, int bwd) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < Nt) {
        const int g = gt_col[t];
        float x = __uint_as_float(0x7fc00000u);
        if (g >= 0 && g < Nv) {
            x = score[(int64_t)t * ld + g];
            if constexpr (DUAL) x = ret_dual_val(x, k, lse_col[g], (float)Nt);
        }
        xg[t] = x;
    }
    if (bwd && t < Nv) {
        int lo = col_ptr[t], hi = col_ptr[t + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > nnz ? nnz : hi;
        float best = 0.f;
        int ib = -1;
        for (int r = lo; r < hi; ++r) {
            const int i = col_rows[r];
            if (i < 0 || i >= Nt) continue;
            float y = score[(int64_t)i * ld + t];
            if constexpr (DUAL) y = ret_dual_val(y, k, lse_row[i], (float)Nv);
            if (ib < 0 || y > best || (y == best && i < ib)) { best = y; ib = i; }
        }
        col_m[t] = best;
        col_i[t] = ib;
    }
}

// ---------------------------------------------------------------- the rank pass
template <bool VEC4, bool DUAL, bool BWD>
__global__ __launch_bounds__(256) void ret_rank_kernel(const float* __restrict__ score, int64_t ld, const int* __restrict__ gt_col, float k,
                                                       const float* __restrict__ lse_row, const float* __restrict__ lse_col,
                                                       const float* __restrict__ xg, const float* __restrict__ col_m,
                                                       const int* __restrict__ col_i, int* __restrict__ rank_f, int* __restrict__ part_cnt,
                                                       int Nt, int Nv) {
    // Row state is wave-uniform and lives in scalar registers: the threshold / ground-truth column / lse of a row come from uniform
    // addresses, and a row's count is the population count of the compare mask (v_cmp writes the mask, the scalar unit counts and adds).
    __shared__ int sh_cnt[RT_WAVES][RT_ROWS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i0 = blockIdx.x * RT_ROWS;
    int cnt[RT_ROWS];
#pragma unroll
    for (int r = 0; r < RT_ROWS; ++r) cnt[r] = 0;
    const float fNt = (float)Nt, fNv = (float)Nv;
    const int nchunk = (Nv + RT_COLS - 1) / RT_COLS;
    for (int c = wave; c < nchunk; c += RT_WAVES) {
        const int j0 = c * RT_COLS;
        float lc[4], cm[4];
        int ci[4], cc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = ret_col<VEC4>(j0, lane, e);
            const bool in = j < Nv;
            lc[e] = (DUAL && in) ? lse_col[j] : 0.f;
            cm[e] = (BWD && in) ? col_m[j] : 0.f;
            ci[e] = (BWD && in) ? col_i[j] : -1;
            cc[e] = 0;
        }
#pragma unroll
        for (int rg = 0; rg < RT_ROWS / 8; ++rg) {
            float v[8][4];
#pragma unroll
            for (int r = 0; r < 8; ++r) ret_load4<VEC4>(score, ld, i0 + rg * 8 + r, Nt, j0, lane, Nv, v[r]);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int rr = rg * 8 + r, i = i0 + rr;
                const int ic = i < Nt ? i : Nt - 1;             // rows past the end load nothing (NaN values): any valid address will do
                const float t = xg[ic];
                const int g = gt_col[ic];
                float lr = 0.f;
                if constexpr (DUAL && BWD) lr = lse_row[ic];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = ret_col<VEC4>(j0, lane, e);
                    const float s = v[r][e];                    // NaN outside the matrix: every compare below is false
                    const float x = DUAL ? ret_dual_val(s, k, lc[e], fNt) : s;
                    cnt[rr] += __popcll(__ballot(x > t || (x == t && j < g)));
                    if constexpr (BWD) {
                        const float y = DUAL ? ret_dual_val(s, k, lr, fNv) : s;
                        cc[e] += (y > cm[e] || (y == cm[e] && i < ci[e])) ? 1 : 0;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);          // as in ret_stats_kernel
        }
        if constexpr (BWD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = ret_col<VEC4>(j0, lane, e);
                if (j < Nv) part_cnt[(int64_t)blockIdx.x * Nv + j] = cc[e];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RT_ROWS; ++r) sh_cnt[wave][r] = cnt[r];
    }
    __syncthreads();
    if (threadIdx.x < RT_ROWS && i0 + (int)threadIdx.x < Nt) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < RT_WAVES; ++w) n += sh_cnt[w][threadIdx.x];
        const int g = gt_col[i0 + threadIdx.x];
        rank_f[i0 + threadIdx.x] = (g >= 0 && g < Nv) ? n : -1;
    }
}

__global__ __launch_bounds__(256) void ret_rank_finalize_kernel(const int* __restrict__ part_cnt, const int* __restrict__ col_i,
                                                                int* __restrict__ rank_b, int nblk, int Nv) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Nv) return;
    int n = 0;
    for (int b = 0; b < nblk; ++b) n += part_cnt[(int64_t)b * Nv + j];
    rank_b[j] = col_i[j] >= 0 ? n : -1;
}

// ---------------------------------------------------------------- host entries
static inline int64_t ret_align16(int64_t n) { return (n + 15) / 16 * 16; }
// workspace layout, each part 16-byte aligned: [partial A: nblk * Nv floats | partial B: the same | xg, lse2_row: Nt floats each |
// col_m, lse2_col: Nv floats each | col_i: Nv ints]
static int64_t ret_workspace(int Nt, int Nv) {
    const int64_t nblk = (Nt + RT_ROWS - 1) / RT_ROWS;
    return 2 * ret_align16(nblk * Nv * 4) + 2 * ret_align16((int64_t)Nt * 4) + 3 * ret_align16((int64_t)Nv * 4);
}

extern "C" int valor_retrieval_workspace_bytes(int Nt, int Nv, int64_t* bytes) {
    if (!bytes || Nt < 0 || Nv < 0) return VALOR_ERR_ARG;
    *bytes = (Nt == 0 || Nv == 0) ? 0 : ret_workspace(Nt, Nv);
    return VALOR_OK;
}

extern "C" int valor_retrieval_ranks(void* stream, const float* score, int64_t ld, const int* gt_col, const int* col_ptr,
                                     const int* col_rows, int nnz, float inv_temp, int dual, float* lse_row, float* lse_col, int* rank_f,
                                     int* rank_b, void* workspace, int64_t workspace_bytes, int Nt, int Nv) {
    if (Nt <= 0 || Nv <= 0) return VALOR_OK;
    const bool bwd = rank_b != nullptr;
    if (!score || !gt_col || !rank_f || !workspace || ld < Nv) return VALOR_ERR_ARG;
    if (bwd && (!col_ptr || !col_rows || nnz < 0)) return VALOR_ERR_ARG;
    if (dual && (!(inv_temp > 0.f) || !isfinite(inv_temp))) return VALOR_ERR_ARG;
    if (((uintptr_t)score & 3) || ((uintptr_t)gt_col & 3) || ((uintptr_t)col_ptr & 3) || ((uintptr_t)col_rows & 3) || ((uintptr_t)lse_row & 3) ||
        ((uintptr_t)lse_col & 3) || ((uintptr_t)rank_f & 3) || ((uintptr_t)rank_b & 3) || ((uintptr_t)workspace & 15))
        return VALOR_ERR_ARG;
    if (workspace_bytes < ret_workspace(Nt, Nv)) return VALOR_ERR_ARG;
    const int nblk = (Nt + RT_ROWS - 1) / RT_ROWS;
    char* ws = (char*)workspace;
    float* partA = (float*)ws;            ws += ret_align16((int64_t)nblk * Nv * 4);
    float* partB = (float*)ws;            ws += ret_align16((int64_t)nblk * Nv * 4);
    float* xg = (float*)ws;               ws += ret_align16((int64_t)Nt * 4);
    float* l2row = (float*)ws;            ws += ret_align16((int64_t)Nt * 4);
    float* col_m = (float*)ws;            ws += ret_align16((int64_t)Nv * 4);
    float* l2col = (float*)ws;            ws += ret_align16((int64_t)Nv * 4);
    int* col_i = (int*)ws;
    const float k2 = (float)((double)inv_temp * 1.4426950408889634);
    const bool vec4 = (ld % 4) == 0 && ((uintptr_t)score & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 blk(256), gcol((Nv + 255) / 256), gthr(((Nt > Nv ? Nt : Nv) + 255) / 256);
    if (dual) {
        if (vec4) hipLaunchKernelGGL(ret_stats_kernel<true>, dim3(nblk), blk, 0, st, score, ld, k2, lse_row, l2row, partA, partB, Nt, Nv);
        else hipLaunchKernelGGL(ret_stats_kernel<false>, dim3(nblk), blk, 0, st, score, ld, k2, lse_row, l2row, partA, partB, Nt, Nv);
        hipLaunchKernelGGL(ret_stats_finalize_kernel, gcol, blk, 0, st, (const float*)partA, (const float*)partB, lse_col, l2col, nblk, Nv);
        hipLaunchKernelGGL(ret_thresh_kernel<true>, gthr, blk, 0, st, score, ld, gt_col, col_ptr, col_rows, nnz, k2, (const float*)l2row,
                           (const float*)l2col, xg, col_m, col_i, Nt, Nv, (int)bwd);
    } else {
        hipLaunchKernelGGL(ret_thresh_kernel<false>, gthr, blk, 0, st, score, ld, gt_col, col_ptr, col_rows, nnz, k2, (const float*)l2row,
                           (const float*)l2col, xg, col_m, col_i, Nt, Nv, (int)bwd);
    }
    int* part_cnt = (int*)partA;          // the statistics partials are consumed by now (stream order)
#define RET_RANK(V_, D_, B_)                                                                                                              \
    hipLaunchKernelGGL((ret_rank_kernel<V_, D_, B_>), dim3(nblk), blk, 0, st, score, ld, gt_col, k2, (const float*)l2row,                  \
                       (const float*)l2col, (const float*)xg, (const float*)col_m, (const int*)col_i, rank_f, part_cnt, Nt, Nv)
    switch ((vec4 ? 4 : 0) | (dual ? 2 : 0) | (bwd ? 1 : 0)) {
        case 0: RET_RANK(false, false, false); break;
        case 1: RET_RANK(false, false, true); break;
        case 2: RET_RANK(false, true, false); break;
        case 3: RET_RANK(false, true, true); break;
        case 4: RET_RANK(true, false, false); break;
        case 5: RET_RANK(true, false, true); break;
        case 6: RET_RANK(true, true, false); break;
        default: RET_RANK(true, true, true); break;
    }
#undef RET_RANK
    if (bwd) hipLaunchKernelGGL(ret_rank_finalize_kernel, gcol, blk, 0, st, (const int*)part_cnt, (const int*)col_i, rank_b, nblk, Nv);
    return valor_launch_status();
}
