// Host check of the grouped weight-gradient slice planner (valor_amd/csrc/gemm_group_plan.h), meant for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I valor_amd/csrc tools/gemm_group_plan_check.cpp -o /tmp/plan_check && /tmp/plan_check
// It plans the layers of the benchmarked step, the shapes of tests/test_gemm_group_gpu.py and every group of 1 .. 8 problems drawn from a
// grid of shapes, and asserts for each plan: no empty slice, full slices of at least 6 K-tiles, at most 256 work items when anything is
// split, partial tiles and row-sum partials inside the reported workspace size and not overlapping, the size refused when it does not fit.
#include "gemm_group_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int g_plans = 0;

static void fail(const char* what, const GemmGroupShape* in, int n) {
    fprintf(stderr, "FAIL: %s for the group", what);
    for (int i = 0; i < n; ++i) fprintf(stderr, " %dx%dx%d%s", in[i].M, in[i].N, in[i].K, in[i].rowsum ? "+rs" : "");
    fprintf(stderr, "\n");
    exit(1);
}

static void check(const std::vector<GemmGroupShape>& g, int esz, bool print = false) {
    const int n = (int)g.size();
    GemmGroupSlice out[VALOR_GEMM_GROUP];
    int items = -1, kmin = -1;
    int64_t bytes = -1;
    if (gemm_group_plan(g.data(), n, esz, -1, out, &items, &kmin, &bytes) != 0) fail("plan refused", g.data(), n);
    ++g_plans;
    int total_tiles = 0, grid = 0;
    bool split = false;
    int64_t end_prev = 0;
    for (int i = 0; i < n; ++i) {
        const int nk = g[i].K / 64, tiles = ((g[i].M + 255) / 256) * ((g[i].N + 255) / 256);
        const GemmGroupSlice& s = out[i];
        if (s.tiles != tiles) fail("tile count", g.data(), n);
        if (s.slices < 1 || s.ksteps < 1) fail("slice count", g.data(), n);
        if ((int64_t)s.slices * s.ksteps < nk) fail("K not covered", g.data(), n);
        if ((int64_t)(s.slices - 1) * s.ksteps >= nk) fail("empty slice", g.data(), n);
        if (s.slices > 1 && s.ksteps < VALOR_GEMM_GROUP_MIN_KTILES) fail("slices shorter than 6 K-tiles", g.data(), n);
        if (s.slices > 1) {
            split = true;
            if (s.ws_off < end_prev || (s.ws_off & 255)) fail("partial tiles overlap / misaligned", g.data(), n);
            end_prev = s.ws_off + (int64_t)s.slices * g[i].M * g[i].N * esz;
            if (g[i].rowsum) {
                if (s.rs_off < end_prev || (s.rs_off & 255)) fail("row-sum partials overlap / misaligned", g.data(), n);
                end_prev = s.rs_off + (int64_t)s.slices * g[i].M * 4;
            }
            if (end_prev > bytes) fail("workspace overrun", g.data(), n);
        }
        total_tiles += tiles;
        grid += tiles * s.slices;
        if (nk - (s.slices - 1) * s.ksteps < kmin) fail("min K-tiles", g.data(), n);
    }
    if (grid != items) fail("work items", g.data(), n);
    if (split && items > VALOR_GEMM_GROUP_SLOTS) fail("more than 256 work items when splitting", g.data(), n);
    if (!split && bytes != 0) fail("workspace without a split", g.data(), n);
    if (bytes > ((int64_t)65 << 20)) fail("workspace above 65 MiB", g.data(), n);
    if (bytes > 0 && gemm_group_plan(g.data(), n, esz, bytes - 1, out, &items, &kmin, &bytes) == 0) fail("too small a workspace accepted", g.data(), n);
    if (gemm_group_plan(g.data(), n, esz, bytes, out, &items, &kmin, &bytes) != 0) fail("exact workspace refused", g.data(), n);
    if (print) {
        printf("group of %d: %d tiles, %d work items, shortest K loop %d K-tiles, %lld workspace bytes; slices", n, total_tiles, items, kmin, (long long)bytes);
        for (int i = 0; i < n; ++i) printf(" %d", out[i].slices);
        printf("\n");
    }
}

int main() {
    // the benchmarked step: a decoder layer (8832 tokens) and an AST layer (16512 tokens), weights as [out, in], row sums fused
    const int dec[6][2] = {{2304, 768}, {768, 768}, {768, 768}, {768, 768}, {3072, 768}, {768, 3072}};
    const int ast[4][2] = {{2304, 768}, {768, 768}, {3072, 768}, {768, 3072}};
    for (int esz = 2; esz <= 4; esz += 2) {
        std::vector<GemmGroupShape> g;
        for (auto& s : dec) g.push_back({s[0], s[1], 8832, 1});
        check(g, esz, true);
        g.push_back({768, 768, 8832, 1}); g.push_back({2304, 768, 8832, 1});      // a queue that closes at 8: the next layer's first two
        check(g, esz, true);
        g.clear();
        for (auto& s : ast) g.push_back({s[0], s[1], 16512, 1});
        check(g, esz, true);
        for (auto& s : ast) g.push_back({s[0], s[1], 16512, 1});
        check(g, esz, true);
        g.clear();
        g.push_back({768, 768, 8832, 0});
        check(g, esz, true);
    }
    // the test shapes, every group size, equal and mixed K
    const int dims[3] = {256, 320, 768}, ks[3] = {4096, 4160, 8832};
    std::vector<GemmGroupShape> pool;
    for (int m : dims) for (int nn : dims) for (int k : ks) pool.push_back({m, nn, k, (m + nn + k) % 3 == 0});
    unsigned seed = 12345u;
    for (int rep = 0; rep < 20000; ++rep) {
        seed = seed * 1664525u + 1013904223u;
        const int n = 1 + (seed >> 8) % 8;
        std::vector<GemmGroupShape> g;
        for (int i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; g.push_back(pool[(seed >> 8) % pool.size()]); }
        check(g, 2 + 2 * (rep & 1));
    }
    // a wider grid: odd sizes, one-tile and many-tile problems, short and long contractions
    const int wide[7] = {1, 255, 257, 1000, 3072, 4097, 30522}, wk[5] = {64, 384, 4096, 65536, 1048576};
    for (int rep = 0; rep < 20000; ++rep) {
        seed = seed * 1664525u + 1013904223u;
        const int n = 1 + (seed >> 8) % 8;
        std::vector<GemmGroupShape> g;
        for (int i = 0; i < n; ++i) {
            seed = seed * 1664525u + 1013904223u;
            const unsigned r = seed >> 8;
            g.push_back({wide[r % 7], wide[(r / 7) % 7], wk[(r / 49) % 5], (int)((r / 245) & 1)});
        }
        check(g, 2 + 2 * (rep & 1));
    }
    // refused inputs
    GemmGroupSlice out[VALOR_GEMM_GROUP];
    int items, kmin; int64_t bytes;
    GemmGroupShape bad[1] = {{256, 256, 100, 0}};
    if (gemm_group_plan(bad, 1, 2, -1, out, &items, &kmin, &bytes) == 0) { fprintf(stderr, "FAIL: K %% 64 accepted\n"); return 1; }
    if (gemm_group_plan(bad, 0, 2, -1, out, &items, &kmin, &bytes) == 0 || gemm_group_plan(bad, 9, 2, -1, out, &items, &kmin, &bytes) == 0) { fprintf(stderr, "FAIL: n out of range accepted\n"); return 1; }
    printf("%d plans checked\n", g_plans);
    return 0;
}
