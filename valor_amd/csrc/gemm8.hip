// valor_gemm, bf16, large-tile path: 256x256 tile per 512-thread workgroup (8 waves as 2(M) x 4(N), 128x64 outputs
// each = 8x4 v_mfma_f32_16x16x32_bf16 tiles, 128 accumulator VGPRs), BK = 64, one workgroup per CU, and an explicit
// 8-barrier-per-K-tile software pipeline instead of relying on several workgroups per CU to hide each other's loads.
//
// Pipeline (per K-tile "c", 4 phases j = 0..3, each phase = a LOAD segment and a MATH segment separated by s_barrier):
//   LOAD(j): ds_read the register sub-tile(s) of this phase; issue ONE 16 KiB half-tile of LDS-DMA (2 x
//            buffer_load_dwordx4..lds per wave); s_waitcnt vmcnt(8) (this wave's loads of 4 phases ago have landed);
//            s_barrier.
//   MATH(j): 16 MFMAs = one 64x32 quadrant of the wave's 128x64 outputs over K = 64, under s_setprio(1); s_barrier.
//   quadrants  j0: (A'0,B'0)  j1: (A'0,B'1)  j2: (A'1,B'1)  j3: (A'1,B'0)        (B'0 stays in registers j0 -> j3)
//   LDS reads  j0: B'0 + A'0 (12 x ds_read_b128)   j1: B'1 (4)   j2: A'1 (8)   j3: none
//   DMA issue  j0: B'1 of tile c+1   j1: A'1 of c+1   j2: B'0 of c+2   j3: A'0 of c+2
// The waves of the second wave row (waves 4-7, one per SIMD next to a wave 0-3) run ONE barrier late: while one wave
// of a SIMD is in MATH(j) its partner is in LOAD, so the matrix pipe always has exactly one issuing wave per SIMD
// and LDS / DMA issue overlaps the MFMAs of the partner.
//
// LDS: 2 K-tile buffers x 4 half-tiles x 16 KiB = 128 KiB. Half-tile A'h = tile rows [128h, 128h+128), B'h = tile
// columns [128h, 128h+128) (contiguous, so every DMA segment is a full 128-B / 256-B line). The WAVE owns a
// non-contiguous output set instead: rows {128*mh + 64*wm + [0,64)}, columns {128*nh + 32*wn + [0,32)}, i.e. its four
// quadrants (mh, nh) live in the four (A'mh, B'nh) combinations. So a half-tile is consumed by ALL waves in the same
// phase, its LDS slot is dead right after that phase and is re-filled two or three phases later (WAR) for the tile
// two ahead; its data is waited for 4 phases after issue and read at the earliest 5 phases after issue (RAW: own
// vmcnt + a barrier every reader has passed).
// (A persistent variant with DMA look-ahead across tiles and a start skew was built and measured SLOWER: the per-tile
// fixed cost is the epilogue itself -- ~10k cycles of store issue + ~13k of LDS staging -- not the prologue.)
// Half-tile images are the two image formats of gemm.hip (XOR image for k-contiguous operands, rotated [64 k][256 B]
// image + ds_read_b64_tr_b16 for k-slow operands), so all four layouts run on the same schedule.
//
// Requirements (otherwise valor_gemm uses the 128x128 kernels): K % 64 == 0.  M/N tails are handled by the buffer
// range check (zero fill) and masked stores.
#include "gemm_common.h"
#include <stdlib.h>

#define HT_BYTES 16384
#define BUF_BYTES (4 * HT_BYTES)
#define OFF_A0 0
#define OFF_A1 HT_BYTES
#define OFF_B0 (2 * HT_BYTES)
#define OFF_B1 (3 * HT_BYTES)

DEVINL bf16x8_t read_frag_tr8(const char* img, int off, int kk) {
    const char* a = img + off + kk * (32 * 256);
    s16x4_t lo = lds_read_tr4(a), hi = lds_read_tr4(a + 4 * 256);
    return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ASMTR: the transposing reads of the k-slow operands as inline asm (mma.h: tr_issue / tr_wait / tr_frag) -- as compiler builtins
// they drained the counted vmcnt(8) LDS-DMA pipeline three times per K-tile.
// NTS: non-temporal stores of the bf16 outputs (gemm_common.h store_out16; the launcher picks it for short-K problems).
// (A non-temporal A operand -- glds16_nt -- was measured too: it lowers the fabric traffic, not the time; profiles/r03_gemm_l2_ab.json.)
// SCHED 1: software-pipelined K loop (see the loop): no wave-row stagger, two barriers per K-tile, every fragment read and DMA piece between
// two MFMAs of the half-phase before its consumer -- both waves of a SIMD run the same stream and fill each other's issue gaps.
template <bool TA, bool TB, bool ASMTR, bool NTS = false, int SCHED = 0>
__global__ __launch_bounds__(512, 2) void gemm_8ph_kernel(GemmArgs p) {
    const int bid = blockIdx.x;
#include "gemm8_body.h"
}
// valor_gemm_group: the weight gradients of a layer in one launch, each workgroup on the pipelined loop of its own problem
__global__ __launch_bounds__(512, 2) void gemm_8ph_kernel_grp(GemmGroupArgs a) {
    constexpr bool TA = true, TB = true, ASMTR = true, NTS = false;
    constexpr int SCHED = 1;
    int gi = 0;
    while (gi + 1 < a.n && (int)blockIdx.x >= a.first[gi + 1]) ++gi;
    const GemmArgs& p = a.g[gi];
    const int bid = (int)blockIdx.x - a.first[gi];
#include "gemm8_body.h"
}

// inline-asm transposing reads in the k-slow 8-phase kernels (see ASMTR above); VALOR_GEMM_TR_ASM=0/1 presets it for A/B runs
static int g_8ph_tr_asm = [] { const char* e = getenv("VALOR_GEMM_TR_ASM"); return e ? atoi(e) : 1; }();
extern "C" int valor_gemm_set_tr_asm(int v) {
    const int old = g_8ph_tr_asm;
    if (v >= 0) g_8ph_tr_asm = v;
    return old;
}

// one-pass bf16 epilogue for plain problems; VALOR_GEMM_FAST_EPI=0/1 presets it
static int g_8ph_fast_epi = [] { const char* e = getenv("VALOR_GEMM_FAST_EPI"); return e ? atoi(e) : 1; }();
extern "C" int valor_gemm_set_fast_epilogue(int v) {
    const int old = g_8ph_fast_epi;
    if (v >= 0) g_8ph_fast_epi = v;
    return old;
}

// K-loop schedule of the 256x256 kernel: 0 = eight barriers per K-tile with the wave rows staggered, 1 = software-pipelined (two barriers);
// VALOR_GEMM_8PH_SCHED presets it
// 1000 (default) = per problem: pipelined for forward / dgrad contractions of K >= 2048 (+4 .. +11 % on the K = 2304 / 3072 ViT shapes, 0.94 ..
// 1.0 at K = 768 / 1536) and for wgrads whose K-slices are short (<= 48 K-tiles per workgroup: +2 .. +6 % on the decoder / AST wgrads; the
// 225-tile slices of the ViT wgrads run 0.88 .. 0.93 pipelined) -- profiles/r04_gemm_narrow_ab_v4.json
static int g_8ph_sched = [] { const char* e = getenv("VALOR_GEMM_8PH_SCHED"); return e ? atoi(e) : 1000; }();
extern "C" int valor_gemm_set_8ph_sched(int v) {
    const int old = g_8ph_sched;
    if (v == 0 || v == 1 || v == 1000) g_8ph_sched = v;
    return old;
}

int gemm_tr_asm_now() { return GEMM_KNOB(tr_asm, g_8ph_tr_asm); }
int gemm_fast_epilogue_now() { return GEMM_KNOB(fast_epilogue, g_8ph_fast_epi); }

void launch_gemm_8ph(hipStream_t st, int transA, int transB, const GemmArgs& p_in) {
    GemmArgs p = p_in;
    const int fast_epi_ = gemm_fast_epilogue_now(), tr_asm_ = gemm_tr_asm_now();
    // measured (profiles/r02_gemm_epilogue_ab.json): the bf16 tile epilogue wins 1-5 % on plain / bias / activation / C += problems,
    // loses on a pre-activation copy (two tile passes: 939 vs 741 us on the ViT fc1 forward) and on the act' multiply (927 vs 896 us):
    // those keep the general epilogue (mode 2 forces the tile path everywhere it is implemented, for tests / A-B runs)
    const bool light_dact = p.dact_aux && (p.act & VALOR_ACT_DERIV);          // one multiply per value at read-out
    const bool plainish = fast_epi_ >= 2 || (!p.preact && (!p.dact_aux || light_dact));
    p.fast_epi = fast_epi_ && plainish && !p.out_f32 && p.kslices <= 1 && (p.N & 7) == 0 && (p.ldc & 7) == 0 && !p.rowsum_out &&
                 (!p.dact_aux || (p.ldaux & 7) == 0) && !(p.dact_aux && p.preact) && !transA && !(p.preact && (p.act & VALOR_ACT_DERIV));
    const int tiles_m = (p.M + 255) / 256, tiles_n = (p.N + 255) / 256;
    const int tiles = tiles_m * tiles_n;
    // ---- L2-aware raster (see the kernel): group width from a fabric-traffic model. Per XCD a round = 32 concurrent tiles. Row-major over
    // all tile columns reads A once but, when the weight (tiles_n panels of 256 x K) does not survive a round in the 4 MiB L2 next to the
    // 32 x 128 KiB of output and the A rows, re-fetches every touched panel once per round; with groups of G columns the G panels stay
    // resident and A is read once per group.
    p.raster_g = 0;
    if (p.kslices <= 1 && tiles_n > 1 && gemm_policy(4) != 0) {
        if (gemm_policy(4) != 1000) {
            p.raster_g = gemm_policy(4) < tiles_n ? gemm_policy(4) : 0;
        } else {
            const double panel = 256.0 * p.K * 2.0, a_bytes = (double)p.M * p.K * 2.0, rounds = tiles / 256.0;
            const double resident = 2.5 * 1048576.0;
            const int touched = tiles_n < 32 ? tiles_n : 32;
            double best = a_bytes + (tiles_n * panel <= resident ? 8.0 * tiles_n * panel : (rounds < 1.0 ? 1.0 : rounds) * 8.0 * touched * panel);
            for (int ng = 2; ng <= tiles_n; ++ng) {
                const int G = (tiles_n + ng - 1) / ng;
                if (G * panel > resident) continue;
                const double cost = ng * a_bytes + 8.0 * tiles_n * panel;
                if (cost < 0.9 * best) { best = cost; p.raster_g = G; }     // only for a clear win: grouping shortens the A rows' reuse window
            }
        }
    }
    // non-temporal output stores: bf16 outputs of short-K problems (policy key 5: 0 never, 1 always, 1000 = K <= 1024)
    const bool nts = !transA && !p.out_f32 && p.kslices <= 1 && (gemm_policy(5) == 1 || (gemm_policy(5) == 1000 && p.K <= 1024));
    p.st_mode = nts ? 1 : 0;
    dim3 grid(tiles * (p.kslices > 1 ? p.kslices : 1));
    const size_t lds = 2 * BUF_BYTES;
    int sched = GEMM_KNOB(sched_256, g_8ph_sched);
    if (sched == 1000) {
        const int ktiles = p.kslices > 1 ? p.ksteps_per_slice : p.K / 64;
        sched = transA ? (ktiles <= 48 ? 1 : 0) : (p.K >= 2048 ? 1 : 0);
    }
#define VALOR_8PH_LAUNCH(TA_, TB_, NTS_)                                                                        \
    do {                                                                                                        \
        static bool attr_set = false;                                                                           \
        constexpr bool kslow_ = TA_ || TB_;                                                                     \
        if (!attr_set) {                                                                                        \
            hipFuncSetAttribute((const void*)gemm_8ph_kernel<TA_, TB_, false, NTS_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipFuncSetAttribute((const void*)gemm_8ph_kernel<TA_, TB_, true, NTS_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipFuncSetAttribute((const void*)gemm_8ph_kernel<TA_, TB_, kslow_, NTS_, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            attr_set = true;                                                                                    \
        }                                                                                                       \
        if (sched == 1 && (tr_asm_ || !kslow_)) hipLaunchKernelGGL((gemm_8ph_kernel<TA_, TB_, kslow_, NTS_, 1>), grid, dim3(512), lds, st, p); \
        else if (tr_asm_ && kslow_) hipLaunchKernelGGL((gemm_8ph_kernel<TA_, TB_, true, NTS_>), grid, dim3(512), lds, st, p); \
        else hipLaunchKernelGGL((gemm_8ph_kernel<TA_, TB_, false, NTS_>), grid, dim3(512), lds, st, p);       \
    } while (0)
    if (!transA && !transB) { if (nts) VALOR_8PH_LAUNCH(false, false, true); else VALOR_8PH_LAUNCH(false, false, false); }
    else if (!transA && transB) { if (nts) VALOR_8PH_LAUNCH(false, true, true); else VALOR_8PH_LAUNCH(false, true, false); }
    else if (transA && !transB) VALOR_8PH_LAUNCH(true, false, false);
    else VALOR_8PH_LAUNCH(true, true, false);
#undef VALOR_8PH_LAUNCH
}

void launch_gemm_8ph_group(hipStream_t st, const GemmGroupArgs& a) {
    const size_t lds = 2 * BUF_BYTES;
    static bool attr_set = false;
    if (!attr_set) {
        hipFuncSetAttribute((const void*)gemm_8ph_kernel_grp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL(gemm_8ph_kernel_grp, dim3(a.first[a.n]), dim3(512), lds, st, a);
}
