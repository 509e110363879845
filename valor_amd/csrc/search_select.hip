// Retrieval search: valor_topk_rows (search.hip) with a column filter and one result per group (valor_amd/search.py RetrievalIndex:
// removed clips, where=, collapse=). See include/valor_hip.h for the contract.
//
// The total order, the key (ord, idx), the two launches, the segment plan and the workspace are search.hip's (topk.h). Two additions:
//   keep    a candidate whose keep byte is 0 never enters the accumulator. The byte is read only for a candidate that beats the
//           threshold: after the first thousand columns that is a few loads per step, not one per column.
//   group   the accumulator carries a third column, the candidate's group id (-1: a group of its own). Members of one group are ONE
//           result, represented by the group's best member. A compaction sorts the buffer best first, drops every entry whose group
//           id already appeared EARLIER in sorted order (that earlier entry is the better member), moves the survivors to the front
//           in order and keeps k. The threshold is the k-th survivor, and only if k survivors exist: k distinct groups then hold a
//           better representative than anything below it, which is what makes pruning exact. A buffer with fewer than k distinct
//           groups has no threshold (a k-th entry that is some group's second member would prune a third group's only member).
//           Members of one group meet in one segment, across segments and across merges; each time they go through the same
//           compaction, so a later, better member replaces the representative and a later, worse one vanishes. The merge kernel reads
//           the group of every key (segment partials and the entries already in top_idx alike) through `group` by the key's index.
// The accumulator is search.hip's, one template in topk.h: TkState<GROUPED> carries the third column and tk_compact<true> the
// de-duplication (an all-pairs scan over the sorted buffer, survivors placed by a ballot prefix sum). After a compaction at most
// k <= 256 of the 512 slots are taken and slots 0 .. cnt - 1 are all written, as tk_push requires. The kernels are instantiated with
// and without GROUPED: without `group` the compaction is valor_topk_rows': sort, keep k.
#include "topk.h"

template <bool VEC4, bool GROUPED>
__global__ __launch_bounds__(TK_THREADS) void topk_select_segment_kernel(const float* __restrict__ score, int64_t ld, int C, int64_t col_base,
                                                                         int k, int nseg, int seg, const uint8_t* __restrict__ keep,
                                                                         int64_t keep_ld, const int32_t* __restrict__ group, int64_t group_ld,
                                                                         uint32_t* __restrict__ part_ord, int64_t* __restrict__ part_idx) {
    __shared__ int64_t sh_idx[TK_CAP];
    __shared__ __attribute__((aligned(16))) int sh_grp[TK_CAP];
    __shared__ uint32_t sh_ord[TK_CAP];
    __shared__ int sh_cnt, sh_wsum[TK_THREADS / 64];
    const int r = blockIdx.x / nseg, sg = blockIdx.x % nseg;
    const float* row = score + (int64_t)r * ld;
    const uint8_t* keep_row = keep ? keep + (int64_t)r * keep_ld : nullptr;
    const int32_t* group_row = GROUPED ? group + (int64_t)r * group_ld : nullptr;    // GROUPED: group != NULL
    const int64_t c0 = (int64_t)sg * seg;
    const int64_t c1 = (c0 + seg < C) ? c0 + seg : C;
    TkState<GROUPED> s;
    tk_init(s, sh_ord, sh_idx, &sh_cnt, k, sh_grp, sh_wsum);
    float cur[4], nxt[4] = {0.f, 0.f, 0.f, 0.f};
    tk_load4<VEC4>(row, c0, (int)c1, cur);
    for (int64_t j0 = c0; j0 < c1; j0 += TK_STEP) {
        if (j0 + TK_STEP < c1) tk_load4<VEC4>(row, j0 + TK_STEP, (int)c1, nxt);
        uint32_t o[4];
        int64_t ix[4];
        int g[4];
        bool w[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t j = tk_col<VEC4>(j0, e);
            o[e] = tk_ord(cur[e]);
            ix[e] = col_base + j;
            w[e] = j < c1 && tk_beats(o[e], ix[e], s.thr_o, s.thr_i);
            if (w[e] && keep_row) w[e] = keep_row[ix[e]] != 0;          // j < C: inside the arrays the caller sized for col_base + C
            g[e] = (w[e] && group_row) ? group_row[ix[e]] : -1;
            any = any || w[e];
        }
        if (__syncthreads_or(any)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) tk_push(s, w[e] && tk_beats(o[e], ix[e], s.thr_o, s.thr_i), o[e], ix[e], g[e]);
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

template <bool GROUPED>
__global__ __launch_bounds__(TK_THREADS) void topk_select_merge_kernel(const uint32_t* __restrict__ part_ord, const int64_t* __restrict__ part_idx,
                                                                       int npart, int k, int merge, const uint8_t* __restrict__ keep,
                                                                       int64_t keep_ld, const int32_t* __restrict__ group, int64_t group_ld,
                                                                       float* __restrict__ top_val, int64_t* __restrict__ top_idx) {
    __shared__ int64_t sh_idx[TK_CAP];
    __shared__ __attribute__((aligned(16))) int sh_grp[TK_CAP];
    __shared__ uint32_t sh_ord[TK_CAP];
    __shared__ int sh_cnt, sh_wsum[TK_THREADS / 64];
    const int r = blockIdx.x;
    const uint8_t* keep_row = keep ? keep + (int64_t)r * keep_ld : nullptr;
    const int32_t* group_row = GROUPED ? group + (int64_t)r * group_ld : nullptr;    // GROUPED: group != NULL
    TkState<GROUPED> s;
    tk_init(s, sh_ord, sh_idx, &sh_cnt, k, sh_grp, sh_wsum);
    if (merge) {                        // k <= 256: one entry per thread; an entry the filter no longer admits is dropped here
        const int p = threadIdx.x;
        uint32_t o = 0u;
        int64_t i = -1;
        if (p < k) {
            i = top_idx[(int64_t)r * k + p];
            o = tk_ord(top_val[(int64_t)r * k + p]);
        }
        bool want = i >= 0 && i != TK_NONE;
        if (want && keep_row) want = keep_row[i] != 0;
        tk_push(s, want, o, i, (want && group_row) ? group_row[i] : -1);
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
        const bool want = tk_beats(o, i, s.thr_o, s.thr_i);             // false for the sentinel: nothing is read through it
        tk_push(s, want, o, i, (want && group_row) ? group_row[i] : -1);
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
extern "C" int valor_topk_select_workspace_bytes(int R, int C, int k, int64_t* bytes) {
    if (!bytes || R < 0 || C < 0 || k < 1 || k > 256) return VALOR_ERR_ARG;
    *bytes = R == 0 ? 0 : tk_workspace(R, C, k);
    return VALOR_OK;
}

template <bool GROUPED>
static void ts_launch(hipStream_t st, bool vec4, int R, int nseg, int seg, const float* score, int64_t ld, int C, int64_t col_base, int k, int merge,
                      const uint8_t* keep, int64_t keep_ld, const int32_t* group, int64_t group_ld, uint32_t* part_ord, int64_t* part_idx,
                      float* top_val, int64_t* top_idx) {
    const dim3 blk(TK_THREADS), grid((unsigned)(R * nseg));
    if (vec4)
        hipLaunchKernelGGL((topk_select_segment_kernel<true, GROUPED>), grid, blk, 0, st, score, ld, C, col_base, k, nseg, seg, keep, keep_ld, group,
                           group_ld, part_ord, part_idx);
    else
        hipLaunchKernelGGL((topk_select_segment_kernel<false, GROUPED>), grid, blk, 0, st, score, ld, C, col_base, k, nseg, seg, keep, keep_ld, group,
                           group_ld, part_ord, part_idx);
    hipLaunchKernelGGL((topk_select_merge_kernel<GROUPED>), dim3((unsigned)R), blk, 0, st, (const uint32_t*)part_ord, (const int64_t*)part_idx, nseg * k,
                       k, merge, keep, keep_ld, group, group_ld, top_val, top_idx);
}

extern "C" int valor_topk_rows_select(void* stream, const float* score, int64_t ld, int R, int C, int64_t col_base, int k, int merge,
                                      const uint8_t* keep, int64_t keep_ld, const int32_t* group, int64_t group_ld, float* top_val,
                                      int64_t* top_idx, void* workspace, int64_t workspace_bytes) {
    if (R == 0) return VALOR_OK;
    if (R < 0 || C < 0 || k < 1 || k > 256 || ld < C) return VALOR_ERR_ARG;
    if ((!score && C > 0) || !top_val || !top_idx || !workspace) return VALOR_ERR_ARG;          // no columns: nothing is read through score
    if (col_base < 0 || col_base > INT64_MAX - 1 - (int64_t)C) return VALOR_ERR_ARG;        // INT64_MAX is the missing-candidate sentinel
    if (((uintptr_t)score & 3) || ((uintptr_t)top_val & 3) || ((uintptr_t)top_idx & 7) || ((uintptr_t)workspace & 15)) return VALOR_ERR_ARG;
    if (keep_ld < 0 || group_ld < 0 || ((uintptr_t)group & 3)) return VALOR_ERR_ARG;
    if (workspace_bytes < tk_workspace(R, C, k)) return VALOR_ERR_ARG;
    int nseg, seg;
    tk_plan(R, C, &nseg, &seg);
    if ((int64_t)R * nseg > INT32_MAX) return VALOR_ERR_ARG;
    const int64_t n = (int64_t)R * nseg * k;
    int64_t* part_idx = (int64_t*)workspace;
    uint32_t* part_ord = (uint32_t*)((char*)workspace + tk_align16(n * 8));
    const bool vec4 = (ld % 4) == 0 && ((uintptr_t)score & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (group) ts_launch<true>(st, vec4, R, nseg, seg, score, ld, C, col_base, k, merge, keep, keep_ld, group, group_ld, part_ord, part_idx, top_val, top_idx);
    else ts_launch<false>(st, vec4, R, nseg, seg, score, ld, C, col_base, k, merge, keep, keep_ld, group, group_ld, part_ord, part_idx, top_val, top_idx);
    return valor_launch_status();
}
