// Slice plan of a grouped weight-gradient launch (valor_gemm_group, gemm.hip). Host code without a HIP dependency: gemm.hip includes it,
// and tools/gemm_group_plan_check.cpp runs it under the host sanitizers over the step's shapes.
//
// A group is up to 8 bf16 products C_i += A_i^T . B_i on the 256x256 tile (family 3), issued as ONE launch whose 1-D grid is the
// concatenation of the problems' (slice, tile) items. Problem i gets S_i K-slices such that
//   * sum_i tiles_i * S_i fits ONE round of the 256 workgroup slots (one 256x256 workgroup per CU),
//   * no workgroup gets fewer than 6 K-tiles and no slice is empty,
//   * K-tiles per workgroup are as equal as the integers allow: the plan is the smallest common K-tile count kt >= 6 for which
//     S_i = ceil(nk_i / kt) fits the round -- with equal K one common S, with different K S_i proportional to nk_i.
// A group whose tiles alone fill more than half a round cannot be split (S = 2 would not fit): it runs unsplit and accumulates straight
// into C, no reduction at all. The plan is a pure function of the shapes in the group.
#pragma once
#include <stdint.h>

#define VALOR_GEMM_GROUP 8
#define VALOR_GEMM_GROUP_SLOTS 256
#define VALOR_GEMM_GROUP_MIN_KTILES 6

struct GemmGroupShape { int M, N, K; int rowsum; };
struct GemmGroupSlice {
    int tiles;            // 256x256 output tiles
    int slices;           // S_i (1 = unsplit: the kernel's own epilogue writes C)
    int ksteps;           // K-tiles per slice (the last slice may be shorter, never empty)
    int64_t ws_off;       // byte offset of the [S][M][N] partial tiles in the group's workspace (S > 1)
    int64_t rs_off;       // byte offset of the [S][M] fp32 row-sum partials (S > 1 and rowsum)
};

static inline int64_t gemm_group_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

// Returns 0 and fills out[0 .. n) / *items (grid size) / *min_ktiles (shortest K loop of any workgroup) / *bytes (workspace used), or -1:
// n out of range, a shape the 256x256 kernel does not take (K % 64, K < 64), or a workspace of `ws_bytes` too small for the partial
// tiles (partial_esz = 2: bf16 partials, 4: fp32). The caller may pass ws_bytes = -1 to ask for the size only.
static inline int gemm_group_plan(const GemmGroupShape* in, int n, int partial_esz, int64_t ws_bytes, GemmGroupSlice* out, int* items,
                                  int* min_ktiles, int64_t* bytes) {
    if (n < 1 || n > VALOR_GEMM_GROUP || (partial_esz != 2 && partial_esz != 4)) return -1;
    int total = 0, nk_max = 0;
    for (int i = 0; i < n; ++i) {
        if (in[i].M <= 0 || in[i].N <= 0 || in[i].K < 64 || (in[i].K % 64) != 0) return -1;
        const int64_t t = (int64_t)((in[i].M + 255) / 256) * ((in[i].N + 255) / 256);
        if (t > (1 << 20)) return -1;
        out[i].tiles = (int)t;
        total += (int)t;
        if (total > (1 << 24)) return -1;
        const int nk = in[i].K / 64;
        if (nk > nk_max) nk_max = nk;
    }
    // the smallest kt >= 6 whose slice counts fit the round; kt = nk_max is the unsplit plan (every S_i = 1)
    int kt = nk_max;
    if (2 * total <= VALOR_GEMM_GROUP_SLOTS) {
        for (int c = VALOR_GEMM_GROUP_MIN_KTILES; c < nk_max; ++c) {
            int64_t need = 0;
            for (int i = 0; i < n; ++i) need += (int64_t)out[i].tiles * ((in[i].K / 64 + c - 1) / c);
            if (need <= VALOR_GEMM_GROUP_SLOTS) { kt = c; break; }
        }
    }
    int64_t off = 0;
    int grid = 0, kmin = 1 << 30;
    for (int i = 0; i < n; ++i) {
        const int nk = in[i].K / 64;
        int s = (nk + kt - 1) / kt;
        if (s > nk / VALOR_GEMM_GROUP_MIN_KTILES) s = nk / VALOR_GEMM_GROUP_MIN_KTILES;     // full slices of at least 6 K-tiles
        if (s < 1) s = 1;
        int steps = (nk + s - 1) / s;            // equalise inside the problem,
        s = (nk + steps - 1) / steps;            // then drop what would be an empty trailing slice
        out[i].slices = s;
        out[i].ksteps = steps;
        out[i].ws_off = out[i].rs_off = 0;
        if (s > 1) {
            out[i].ws_off = off;
            off += gemm_group_align((int64_t)s * in[i].M * in[i].N * partial_esz);
            if (in[i].rowsum) {
                out[i].rs_off = off;
                off += gemm_group_align((int64_t)s * in[i].M * 4);
            }
        }
        grid += out[i].tiles * s;
        const int last = nk - (s - 1) * steps;   // K-tiles of the last slice: 1 .. steps
        if (last < kmin) kmin = last;
    }
    if (ws_bytes >= 0 && off > ws_bytes) return -1;
    *items = grid; *min_ktiles = kmin; *bytes = off;
    return 0;
}
