// Retrieval search: the k best columns of every row of a score matrix, streaming (valor_amd/search.py RetrievalIndex walks a clip bank in
// chunks and folds each chunk's [queries, chunk] scores into a running [queries, k] result). See include/valor_hip.h for the contract.
//
// ONE total order decides everything: a candidate is the pair (value, global index); value descending, then index ascending; a NaN below
// every number. The value is mapped to an orderable uint32 (NaN -> 0, -0 -> +0, otherwise the usual sign flip), so a candidate is the key
// (ord, idx) and "a beats b" is ord_a > ord_b || (ord_a == ord_b && idx_a < idx_b). Indices are unique, hence keys are: the k best of a
// set are ONE set, whatever order lanes, waves and workgroups met them in. No float atomics, no float arithmetic at all.
//
// Two launches:
//   topk_segment_kernel  grid = rows x column segments (a segment is a multiple of 1024 columns, chosen on the host so that one row of a
//                        long chunk still spreads over the machine). A workgroup of four waves streams its segment, 1024 columns a step
//                        (16-byte loads, the next step's load in flight), through the accumulator below and writes its k best keys to
//                        the workspace.
//   topk_merge_kernel    one workgroup per row: the segments' keys and, with merge, the k entries already in top_val / top_idx go
//                        through the same accumulator; the k best are written back as value / index (-inf / -1 for a missing one).
//
// The accumulator (csrc/topk.h, shared with search_select.hip): TK_CAP = 512 keys in LDS (6 KB), a counter, and the running k-th best as a threshold in registers. A lane whose key
// beats the threshold takes a slot (one LDS atomic per wave: ballot, leader add, prefix popcount). When the buffer is full the workgroup
// sorts it (bitonic, best first), keeps the first k, and the k-th becomes the threshold; lanes that found no slot try again unless the
// new threshold rules them out. Pruning against the k-th best of a subset is exact. After the first thousand columns few keys pass (k / n
// of them at column n), and a step costs one barrier. The missing-candidate sentinel (0, INT64_MAX) loses to every real key, a NaN's
// included, and is never written as an index: the host refuses col_base + C above INT64_MAX - 1.
#include "topk.h"

template <bool VEC4>
__global__ __launch_bounds__(TK_THREADS) void topk_segment_kernel(const float* __restrict__ score, int64_t ld, int C, int64_t col_base, int k,
                                                                  int nseg, int seg, uint32_t* __restrict__ part_ord,
                                                                  int64_t* __restrict__ part_idx) {
    __shared__ int64_t sh_idx[TK_CAP];
    __shared__ uint32_t sh_ord[TK_CAP];
    __shared__ int sh_cnt;
    const int r = blockIdx.x / nseg, sg = blockIdx.x % nseg;
    const float* row = score + (int64_t)r * ld;
    const int64_t c0 = (int64_t)sg * seg;
    const int64_t c1 = (c0 + seg < C) ? c0 + seg : C;
    TkState<false> s;
    tk_init(s, sh_ord, sh_idx, &sh_cnt, k);
    float cur[4], nxt[4] = {0.f, 0.f, 0.f, 0.f};
    tk_load4<VEC4>(row, c0, (int)c1, cur);
    for (int64_t j0 = c0; j0 < c1; j0 += TK_STEP) {
        if (j0 + TK_STEP < c1) tk_load4<VEC4>(row, j0 + TK_STEP, (int)c1, nxt);
        uint32_t o[4];
        int64_t ix[4];
        bool w[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t j = tk_col<VEC4>(j0, e);
            o[e] = tk_ord(cur[e]);
            ix[e] = col_base + j;
            w[e] = j < c1 && tk_beats(o[e], ix[e], s.thr_o, s.thr_i);
            any = any || w[e];
        }
        if (__syncthreads_or(any)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) tk_push(s, w[e] && tk_beats(o[e], ix[e], s.thr_o, s.thr_i), o[e], ix[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) cur[e] = nxt[e];
    }
    tk_finish(s);
    const int64_t out = ((int64_t)r * nseg + sg) * k;
    for (int p = threadIdx.x; p < k; p += TK_THREADS) {
        part_ord[out + p] = sh_ord[p];
        part_idx[out + p] = sh_idx[p];
    }
}

__global__ __launch_bounds__(TK_THREADS) void topk_merge_kernel(const uint32_t* __restrict__ part_ord, const int64_t* __restrict__ part_idx,
                                                                int npart, int k, int merge, float* __restrict__ top_val,
                                                                int64_t* __restrict__ top_idx) {
    __shared__ int64_t sh_idx[TK_CAP];
    __shared__ uint32_t sh_ord[TK_CAP];
    __shared__ int sh_cnt;
    const int r = blockIdx.x;
    TkState<false> s;
    tk_init(s, sh_ord, sh_idx, &sh_cnt, k);
    if (merge) {                        // k <= 256: one entry per thread
        const int p = threadIdx.x;
        uint32_t o = 0u;
        int64_t i = -1;
        if (p < k) {
            i = top_idx[(int64_t)r * k + p];
            o = tk_ord(top_val[(int64_t)r * k + p]);
        }
        tk_push(s, i >= 0 && i != TK_NONE, o, i);
    }
    const int64_t base = (int64_t)r * npart;
    for (int p0 = 0; p0 < npart; p0 += TK_THREADS) {
        const int p = p0 + threadIdx.x;
        uint32_t o = 0u;
        int64_t i = TK_NONE;
        if (p < npart) {
            o = part_ord[base + p];
            i = part_idx[base + p];
        }
        tk_push(s, tk_beats(o, i, s.thr_o, s.thr_i), o, i);
    }
    tk_finish(s);
    for (int p = threadIdx.x; p < k; p += TK_THREADS) {
        const int64_t i = sh_idx[p];
        const bool real = i != TK_NONE;
        top_val[(int64_t)r * k + p] = real ? tk_val(sh_ord[p]) : -INFINITY;
        top_idx[(int64_t)r * k + p] = real ? i : -1;
    }
}

// ---------------------------------------------------------------- host entries
extern "C" int valor_topk_workspace_bytes(int R, int C, int k, int64_t* bytes) {
    if (!bytes || R < 0 || C < 0 || k < 1 || k > 256) return VALOR_ERR_ARG;
    *bytes = R == 0 ? 0 : tk_workspace(R, C, k);
    return VALOR_OK;
}

extern "C" int valor_topk_rows(void* stream, const float* score, int64_t ld, int R, int C, int64_t col_base, int k, int merge,
                               float* top_val, int64_t* top_idx, void* workspace, int64_t workspace_bytes) {
    if (R == 0) return VALOR_OK;
    if (R < 0 || C < 0 || k < 1 || k > 256 || ld < C) return VALOR_ERR_ARG;
    if ((!score && C > 0) || !top_val || !top_idx || !workspace) return VALOR_ERR_ARG;          // no columns: nothing is read through score
    if (col_base < 0 || col_base > INT64_MAX - 1 - (int64_t)C) return VALOR_ERR_ARG;        // INT64_MAX is the missing-candidate sentinel
    if (((uintptr_t)score & 3) || ((uintptr_t)top_val & 3) || ((uintptr_t)top_idx & 7) || ((uintptr_t)workspace & 15)) return VALOR_ERR_ARG;
    if (workspace_bytes < tk_workspace(R, C, k)) return VALOR_ERR_ARG;
    int nseg, seg;
    tk_plan(R, C, &nseg, &seg);
    if ((int64_t)R * nseg > INT32_MAX) return VALOR_ERR_ARG;
    const int64_t n = (int64_t)R * nseg * k;
    int64_t* part_idx = (int64_t*)workspace;
    uint32_t* part_ord = (uint32_t*)((char*)workspace + tk_align16(n * 8));
    const bool vec4 = (ld % 4) == 0 && ((uintptr_t)score & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 blk(TK_THREADS), grid((unsigned)(R * nseg));
    if (vec4) hipLaunchKernelGGL(topk_segment_kernel<true>, grid, blk, 0, st, score, ld, C, col_base, k, nseg, seg, part_ord, part_idx);
    else hipLaunchKernelGGL(topk_segment_kernel<false>, grid, blk, 0, st, score, ld, C, col_base, k, nseg, seg, part_ord, part_idx);
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)R), blk, 0, st, (const uint32_t*)part_ord, (const int64_t*)part_idx, nseg * k, k,
                       merge, top_val, top_idx);
    return valor_launch_status();
}
