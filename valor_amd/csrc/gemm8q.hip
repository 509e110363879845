// valor_gemm, bf16, the 256x256 tile of gemm8.hip on FOUR waves (256 threads, 2(M) x 2(N)) of 128x128 outputs each: 8x8
// v_mfma_f32_16x16x32_bf16 tiles = 256 accumulator registers per lane, one wave per SIMD (gfx950: 512 registers per lane), one workgroup
// per CU. Same 128 KiB LDS layout (two K-tile buffers of four 16 KiB half-tiles [A'0][A'1][B'0][B'1]), same two image formats, same
// slice-major xcd_remap, same accumulation order per output element as gemm_8ph_kernel: results are bit-identical to it. What changes is
// the LDS read traffic of a K-tile: a wave reads (128 + 128) x 64 x 2 B = 32 KiB of fragments for 128 MFMAs, the CU 128 KiB instead of
// the 192 KiB of eight 128x64 wave tiles (policy key 12).
//
// The WAVE (wm, wn) owns rows {128 mh + 64 wm + [0,64)} x columns {128 nh + 64 wn + [0,64)}, mh, nh in {0,1}: a 64x64 piece of every
// quadrant (A'mh, B'nh), so a half-tile is consumed by all four waves in one phase and its slot is dead right after.
//
// K loop of the k-slow x k-slow layout (the weight gradients, the only layout the launcher is given): EIGHT SLOTS of 16 MFMAs per K-tile,
// slot s = 2 q + kk of quadrant q in the order (0,0) (0,1) (1,0) (1,1), MFMA i = 4 mt + nt. Where the time of the four-phase loop below
// went was measured with cycle stamps and ablation builds (Q8_STAMP / Q8_ABLATE): not in its waits but in ISSUE. An MFMA
// 16x16x32 leaves 8 of its 16 cycles to other instructions, and two transposing reads plus the address add in front of them do not fit.
// So here ONE ds_read_b64_tr_b16 goes behind an MFMA, its half-tile and k-half in the offset field, from eight per-lane address registers
// per buffer that change buffers by 16 adds in the one slot without reads. Register sets as below (FAX = A'0, FAY = A'1, FB0, FB1), by k-halves:
//   slot  MFMAs            reads behind MFMAs 0-7 (s0, s6: 0-15)       DMA behind MFMAs 9, 13   end of slot
//   s0    A'0 k0 x B'0 k0  FB1 k0, k1 <- B'1(c)                        A'0(c+2) 0, 1            -
//   s1    A'0 k1 x B'0 k1  FAY k0 <- A'1(c)                            A'0(c+2) 2, 3            lgkmcnt(8): FB1
//   s2    A'0 k0 x B'1 k0  FAY k1 <- A'1(c)                            B'0(c+2) 0, 1            lgkmcnt(8): FAY k0
//   s3    A'0 k1 x B'1 k1  -                                           B'0(c+2) 2, 3            lgkmcnt(0): FAY k1; vmcnt(16); barrier
//   s4    A'1 k0 x B'0 k0  FAX k0 <- A'0(c+1)                          B'1(c+2) 0, 1            -
//   s5    A'1 k1 x B'0 k1  FAX k1 <- A'0(c+1)                          B'1(c+2) 2, 3            lgkmcnt(8): FAX k0
//   s6    A'1 k0 x B'1 k0  FB0 k0, k1 <- B'0(c+1)                      A'1(c+2) 0, 1            lgkmcnt(15): FAX k1
//   s7    A'1 k1 x B'1 k1  - (the 16 address adds)                     A'1(c+2) 2, 3            lgkmcnt(0): FB0; vmcnt(16); barrier
// Registers: a k-half is read at the earliest in the slot after its last MFMA (FB1 k0 / k1 after s6 / s7, FAY after s6 / s7, FAX k0 / k1
// after s2 / s3, FB0 k0 / k1 after s4 / s5) and first multiplied two slots or more after the slot that read it; the wait that ties it sits one
// slot after its reads and leaves that slot's own reads in flight (LDS reads return in order), so no wait is closer than 9 MFMAs to what it
// waits for, and nothing is in flight where two K-tiles meet. WAR on a half-tile slot: B'1(c) and A'1(c) are read in s0 - s2 and complete
// in every wave at the end of s3, the barrier there opens their refill in s4 - s7; A'0(c+1) and B'0(c+1) are read in s4 - s6 and complete
// at the end of s7, its barrier opens their refill in s0 - s3 of the next K-tile. RAW: pieces go out in the order A'0 B'0 B'1 A'1 of a
// K-tile, two per slot. At the barrier of s3 the 16 youngest pieces of a wave are B'1(c+1), A'1(c+1), A'0(c+2) and B'0(c+2): what is older
// -- A'0(c+1), read from s4, and B'0(c+1), read in s6 -- has landed in every wave behind vmcnt(16) and the barrier; at the barrier of s7 the 16
// youngest are A'0(c+2), B'0(c+2), B'1(c+2) and A'1(c+2), so B'1(c+1) and A'1(c+1), read in s0 - s2 of the next K-tile, have landed.
// The look-ahead is eight slots behind a half-tile's last piece (the four-phase loop: nine). Past the last K-tile a zero-length descriptor keeps
// the counts; the prologue issues K-tiles 0 and 1 in that order and waits for all of K-tile 0.
//
// The other layouts keep the first order of this kernel (nobody launches them): four phases per K-tile, one quadrant of 32 MFMAs each, in
// the order (0,0) (0,1) (1,1) (1,0), MFMA i = 16 kk + 4 mt + nt. With
// one wave per SIMD nobody else fills the issue slots, so every phase carries, BETWEEN its MFMAs, the fragment reads a later phase needs
// and the four 1 KiB LDS-DMA pieces of one half-tile; it ends in lgkmcnt(0), a counted vmcnt and ONE barrier. Four register sets of
// 32 (FAX = A'0, FAY = A'1, FB0, FB1) next to the 256 accumulators; B'0 is multiplied in the first and the last phase, so its set is
// refilled by k-halves: k0 once Q3 is through its k0 MFMAs, k1 at the top of Q0, waited for in the middle of Q0.
//   phase     MFMAs        reads (behind MFMA ..)                                          DMA (slot dead since ..)
//   Q0(c)   (A'0, B'0)     0-3: FB0 k1 <- B'0(c); [15: lgkmcnt(0)]; 16-23: FB1 <- B'1(c)   A'0(c+2)   (read in Q2 / Q3(c-1))
//   Q1(c)   (A'0, B'1)     0-7: FAY <- A'1(c)                                              B'0(c+2)   (read in Q3(c-1) / Q0(c))
//   Q2(c)   (A'1, B'1)     0-3: FAX k0 <- A'0(c+1)                                         B'1(c+2)   (read in Q0(c))
//   Q3(c)   (A'1, B'0)     0-3: FAX k1 <- A'0(c+1); 16-19: FB0 k0 <- B'0(c+1)              A'1(c+2)   (read in Q1(c))
// Counting: every half-tile is first read in the SIXTH phase after the phase that issued it. RAW: the wait at the end of phase p (after
// p's four pieces) leaves the 5 x 4 = 20 pieces of phases p-4 .. p in flight, so what phase p-5 issued has landed in every wave before
// the barrier that opens phase p+1, its reading phase. WAR: the reads of a phase are complete (lgkmcnt(0)) before its closing barrier,
// the refill is issued behind that barrier. Look-ahead past the last K-tile goes through a zero-length descriptor (zero fill, no
// traffic), so the counts hold in the tail; the prologue issues the eight half-tiles the phases before tile 0 would have, in their order.
//
// Epilogue: the general two-pass fp32 epilogue of gemm8.hip (split-K partials, fused row sums, alpha / bias / activation / C += / fp32
// out through epilogue_store8), walked by 256 threads.
// Requirements as for gemm_8ph_kernel: K % 64 == 0; M / N tails by the buffer range check (zero fill) and masked stores.
#include "gemm_common.h"
#include <stdlib.h>
#include <type_traits>

#define HT_BYTES 16384
#define BUF_BYTES (4 * HT_BYTES)
#define OFF_A0 0
#define OFF_A1 HT_BYTES
#define OFF_B0 (2 * HT_BYTES)
#define OFF_B1 (3 * HT_BYTES)

// the registers of one 64-row x 64-k operand piece: fragments (XOR image, ds_read_b128), or the halves of the transposing reads in
// flight (rotated k-slow image, mma.h tr_issue) that become fragments behind the lgkmcnt(0) they are tied to
template <bool KSLOW> struct FragSet;
template <> struct FragSet<false> { bf16x8_t f[4][2]; };
template <> struct FragSet<true> { TrPair f[4][2]; };
DEVINL bf16x8_t frag_of(const bf16x8_t& f) { return f; }
DEVINL bf16x8_t frag_of(const TrPair& t) { return tr_frag(t); }
// The MFMAs as inline asm: the 64 accumulator tiles fill the accumulation half of the register file EXACTLY (256 AGPRs), and only an
// in/out operand tied to that class keeps the register allocator from shuffling tiles between the two halves (the builtin form spilt
// 400 registers here). hipcc pads no hazards around asm: the K loop ends in s_nops before anything reads an accumulator.
DEVINL void mfma_acc(f32x4_t& c, bf16x8_t a, bf16x8_t b) { asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b)); }
// The fused row sums accumulate in ordinary VGPRs. Which two of the four A fragments a wave sums (sel = 1: blocks 0, 1; 2: blocks 2, 3;
// 0: none) is decided INSIDE the asm: a branch in C++ makes the compiler merge the sums with copies right behind the MFMAs, and nothing
// pads the hazard between an MFMA in asm and a VALU read of its result.
DEVINL void mfma_rowsum(f32x4_t& r0, f32x4_t& r1, bf16x8_t ones, bf16x8_t f0, bf16x8_t f1, bf16x8_t f2, bf16x8_t f3, int sel) {
    asm volatile("s_cmp_lt_i32 %7, 1\n\ts_cbranch_scc1 2f\n\ts_cmp_eq_u32 %7, 1\n\ts_cbranch_scc0 1f\n\t"
                 "v_mfma_f32_16x16x32_bf16 %0, %2, %3, %0\n\tv_mfma_f32_16x16x32_bf16 %1, %2, %4, %1\n\ts_branch 2f\n"
                 "1:\n\tv_mfma_f32_16x16x32_bf16 %0, %2, %5, %0\n\tv_mfma_f32_16x16x32_bf16 %1, %2, %6, %1\n"
                 "2:"
                 : "+v"(r0), "+v"(r1) : "v"(ones), "v"(f0), "v"(f1), "v"(f2), "v"(f3), "s"(sel) : "scc");
}
// the reads into a whole set / into its k-half kk are complete
DEVINL void wait8(FragSet<false>&) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
DEVINL void wait8(FragSet<true>& s) { tr_wait8(s.f); }
DEVINL void wait4(FragSet<false>&, int) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
DEVINL void wait4(FragSet<true>& s, int kk) { tr_wait_4(s.f[0][kk], s.f[1][kk], s.f[2][kk], s.f[3][kk]); }

// the reads into k-half kk of a set, issued a slot (16 MFMAs) before the NEWER youngest LDS reads of the wave, are complete: LDS reads return
// in order, so all but those have returned
template <int NEWER> DEVINL void wait4_older(FragSet<true>& s, int kk) {
    asm volatile("s_waitcnt lgkmcnt(%8)" : TR_TIE(s.f[0][kk]), TR_TIE(s.f[1][kk]), TR_TIE(s.f[2][kk]), TR_TIE(s.f[3][kk]) : "n"(NEWER));
}

// f(integral_constant<int, I>) for I = FIRST .. LAST - 1: the index is a constant expression in the body (asm immediates)
template <int FIRST, int LAST, class F> DEVINL void static_for(F&& f) {
    if constexpr (FIRST < LAST) {
        f(std::integral_constant<int, FIRST>{});
        static_for<FIRST + 1, LAST>(f);
    }
}
// ONE transposing read of k-half KK of a set: J = 2 * block + half (0 = lo, 1 = hi) from the per-lane address of that block in its K-tile
// buffer; where the half-tile and the k-half start goes into the instruction's offset field (no address arithmetic in the loop)
template <int HT_OFF, int KK, int J> DEVINL void tr_read1(FragSet<true>& s, const uint32_t (&ad)[4]) {
    if constexpr (J & 1) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(s.f[J >> 1][KK].hi) : "v"(ad[J >> 1]), "n"(HT_OFF + KK * (32 * 256) + 1024));
    else asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(s.f[J >> 1][KK].lo) : "v"(ad[J >> 1]), "n"(HT_OFF + KK * (32 * 256)));
}

#ifdef Q8_STAMP
// diagnostic build only (tools/build_stamp_lib.sh, tools/gemm8q_stamp.py): cycle stamps of every wave, [block][wave][64] uint64 in a buffer of
// their own: [0..5] kernel entry / prologue done / K loop done / drained / epilogue pass 0 / pass 1, [6..7] s_memrealtime around the loop,
// [8] HW_ID, [9] XCC_ID, [10] K-tiles, [11] 1 = slot order, [16..] the boundaries inside K-tile Q8_STAMP_TILE in program order
#define Q8_STAMP_TILE 5
#define Q8_STAMP_BLOCKS 1024
__device__ uint64_t q8_stamp_buf[Q8_STAMP_BLOCKS * 4 * 64];
extern "C" int valor_gemm8q_read_stamps(void* host, int64_t bytes) {
    if (bytes > (int64_t)sizeof(uint64_t) * Q8_STAMP_BLOCKS * 4 * 64) return VALOR_ERR_ARG;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(q8_stamp_buf), (size_t)bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : VALOR_ERR_ARG;
}
#define Q8_AT(i) st_[i] = __builtin_amdgcn_s_memtime()
#define Q8_HS(i) do { if (rel == Q8_STAMP_TILE) hs_[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define Q8_AT(i)
#define Q8_HS(i)
#endif
// ablation builds of the diagnostic library: bit 0 = no DMA in the K loop, bit 1 = no fragment reads in the K loop (results are garbage)
#ifndef Q8_ABLATE
#define Q8_ABLATE 0
#endif

// The k-slow x k-slow layout (the only one the launcher is given today) runs the slot order, the other layouts keep the four phases
// The body takes its problem and its workgroup index `bid` among that problem's work items (gemm8.hip: gemm_8ph_body)
template <bool TA, bool TB>
DEVINL void gemm_8q_body(const GemmArgs& p, const int bid) {
    typedef bf16_t T;
    constexpr bool SLOTS = TA && TB;
#ifdef Q8_STAMP
    uint64_t st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hs_[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) hs_[i] = 0;
    Q8_AT(0);
#endif
    constexpr int BK = 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;

    const int tiles_n = (p.N + 255) >> 8;
    const int tiles_m = (p.M + 255) >> 8;
    int logical, slice = 0;
    if (p.kslices > 1) {
        // work items (K-slice, tile) in slice-major order, a contiguous range per XCD, as in gemm_8ph_kernel
        const int ntiles = tiles_m * tiles_n;
        const int item = xcd_remap(bid, ntiles * p.kslices);
        slice = item / ntiles;
        logical = item - slice * ntiles;
    } else {
        logical = xcd_remap(bid, tiles_m * tiles_n);
    }
    int tm = logical / tiles_n, tn = logical - tm * tiles_n;
    if (p.raster_g > 0 && p.kslices <= 1) {       // L2-aware raster in groups of G tile columns (gemm8.hip)
        const int G = p.raster_g, per = G * tiles_m;
        const int grp = logical / per, w = logical - grp * per;
        const int gw = min(G, tiles_n - grp * G);
        tm = w / gw;
        tn = grp * G + (w - tm * gw);
    }
    const int m0 = tm << 8, n0 = tn << 8;

    const int nk_total = p.K / BK;
    int ks_begin = 0, ks_end = nk_total;
    if (p.kslices > 1) {
        ks_begin = slice * p.ksteps_per_slice;
        ks_end = ks_begin + p.ksteps_per_slice;
        if (ks_end > nk_total) ks_end = nk_total;
        if (ks_begin > nk_total) ks_begin = nk_total;
    }
    const int k_first = ks_begin * BK;
    const int ntile = ks_end - ks_begin;

    f32x4_t acc[8][8];   // [mh*4+mt][nh*4+nt]
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // fused row sums of A (TA only): the tile column 0 workgroups add  ones . A^T  on the matrix pipe, two 16-row blocks per wave and row
    // half (wave wn takes blocks mt = 2 wn, 2 wn + 1): 4 extra MFMAs in phases Q0 and Q2, k0 before k1 like gemm_8ph_kernel
    const bool do_rs = TA && p.rowsum_out != nullptr && tn == 0;
    f32x4_t racc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) racc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    bf16x8_t ones = __builtin_bit_cast(bf16x8_t, (u32x4_t){0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u});
    asm volatile("" : "+v"(ones));           // lives in registers: rematerialised in front of an asm MFMA it would be read too early
    const int rs_sel = __builtin_amdgcn_readfirstlane(do_rs ? wn + 1 : 0);

    // ---- DMA source offsets: half-tile kinds (A'0, A'1, B'0, B'1) x 4 pieces of 1 KiB per wave (piece = wave*4 + i)
    int oA[2][4], oB[2][4];     // [half][i], bumped right behind the load
    int stepA, stepB;
    {
        const int ldA_b = (int)(p.lda * 2), ldB_b = (int)(p.ldb * 2);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int pc = wave * 4 + i;
                if constexpr (!TA) {
                    const int r = pc * 8 + (lane >> 3), c = (lane & 7) ^ ((lane >> 3) & 7);
                    oA[hf][i] = (m0 + hf * 128 + r) * ldA_b + (k_first + c * 8) * 2;
                } else {
                    const int k = pc * 4 + (lane >> 4), s = lane & 15;
                    const int ic = ((s - 2 * (k & 3) - 8 * ((k >> 3) & 1)) & 15) * 8;
                    oA[hf][i] = (k_first + k) * ldA_b + (m0 + hf * 128 + ic) * 2;
                }
                if constexpr (!TB) {
                    const int r = pc * 8 + (lane >> 3), c = (lane & 7) ^ ((lane >> 3) & 7);
                    oB[hf][i] = (n0 + hf * 128 + r) * ldB_b + (k_first + c * 8) * 2;
                } else {
                    const int k = pc * 4 + (lane >> 4), s = lane & 15;
                    const int ic = ((s - 2 * (k & 3) - 8 * ((k >> 3) & 1)) & 15) * 8;
                    oB[hf][i] = (k_first + k) * ldB_b + (n0 + hf * 128 + ic) * 2;
                }
            }
        stepA = TA ? BK * ldA_b : BK * 2;
        stepB = TB ? BK * ldB_b : BK * 2;
    }
    // piece i of half-tile hf of K-tile t into buffer `buf` (zero fill without traffic past the last K-tile), then on to the next K-tile
    auto dmaA = [&](int hf, char* buf, int t, int i) {
        const rsrc_t rs = make_rsrc(p.A, t < ntile ? p.bytesA : 0u);
        glds16(rs, buf + (hf ? OFF_A1 : OFF_A0) + wave * 4096 + i * 1024, oA[hf][i]);
        oA[hf][i] += stepA; asm volatile("" : "+v"(oA[hf][i]));
    };
    auto dmaB = [&](int hf, char* buf, int t, int i) {
        const rsrc_t rs = make_rsrc(p.B, t < ntile ? p.bytesB : 0u);
        glds16(rs, buf + (hf ? OFF_B1 : OFF_B0) + wave * 4096 + i * 1024, oB[hf][i]);
        oB[hf][i] += stepB; asm volatile("" : "+v"(oB[hf][i]));
    };

    // ---- fragment read offsets of the k-slow images: byte offset of the 16-row block (A: wm*4 + mt, B: wn*4 + nt)
    int trA[4], trB[4];
    {
        const int base = (8 * fg + (fr >> 2)) * 256 + 8 * (fr & 1);
        const int rot = 2 * (fr >> 2) + 8 * (fg & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            trA[i] = base + 16 * ((2 * (wm * 4 + i) + ((fr >> 1) & 1) + rot) & 15);
            trB[i] = base + 16 * ((2 * (wn * 4 + i) + ((fr >> 1) & 1) + rot) & 15);
        }
    }
    auto rdA = [&](const char* img, FragSet<TA>& s, int mt, int kk) {
        if constexpr (TA) tr_issue(s.f[mt][kk], img + trA[mt] + kk * (32 * 256));
        else s.f[mt][kk] = read_frag<T>(img, wm * 64 + mt * 16 + fr, kk * 4 + fg);
    };
    auto rdB = [&](const char* img, FragSet<TB>& s, int nt, int kk) {
        if constexpr (TB) tr_issue(s.f[nt][kk], img + trB[nt] + kk * (32 * 256));
        else s.f[nt][kk] = read_frag<T>(img, wn * 64 + nt * 16 + fr, kk * 4 + fg);
    };
#define PIN() __builtin_amdgcn_sched_barrier(0)
    // 32 MFMAs of quadrant (mh, nh) from the sets sa / sb; `slot(i)` is what goes behind MFMA i (reads, DMA pieces, a wait)
    auto quadrant = [&](int mh, int nh, FragSet<TA>& sa, FragSet<TB>& sb, auto&& slot) __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const int i = kk * 16 + mt * 4 + nt;
                    mfma_acc(acc[mh * 4 + mt][nh * 4 + nt], frag_of(sb.f[nt][kk]), frag_of(sa.f[mt][kk]));
                    slot(i);
                    PIN();
                }
    };
    auto rowsum = [&](int hh, FragSet<TA>& sa) __attribute__((always_inline)) {
        if constexpr (TA) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                mfma_rowsum(racc[hh][0], racc[hh][1], ones, frag_of(sa.f[0][kk]), frag_of(sa.f[1][kk]), frag_of(sa.f[2][kk]), frag_of(sa.f[3][kk]), rs_sel);
            PIN();
        }
    };
    // end of a phase (behind the wait for the reads it issued: their registers may be used, their slot may be refilled): what was issued
    // five phases ago has landed, everybody is here
#define PHASE_END()                                                                                               \
    do {                                                                                                          \
        asm volatile("s_waitcnt vmcnt(20)" ::: "memory");                                                         \
        __builtin_amdgcn_s_barrier();                                                                             \
        PIN();                                                                                                    \
    } while (0)

#define LOOP_DMA(...) do { if constexpr (!(Q8_ABLATE & 1)) { __VA_ARGS__; } } while (0)
#define LOOP_RD(...) do { if constexpr (!(Q8_ABLATE & 2)) { __VA_ARGS__; } } while (0)

    FragSet<TA> fax, fay;      // A'0, A'1
    FragSet<TB> fb0, fb1;      // B'0, B'1
    if constexpr (!SLOTS) {
    if (ntile > 0) {
        // prologue = what the phases before tile 0 would have issued, in their order: A'0(0) B'0(0) B'1(0) A'1(0) A'0(1) B'0(1) B'1(1)
        // A'1(1) = 32 pieces; with 20 in flight A'0(0), B'0(0) and B'1(0) have landed
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            char* const b = smem + t * BUF_BYTES;
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaA(0, b, t, i);
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaB(0, b, t, i);
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaB(1, b, t, i);
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaA(1, b, t, i);
        }
        PIN();
        PHASE_END();
        // what Q2 / Q3 of a tile before the first would have read; the barrier behind it is the one that lets Q0(0) refill A'0
#pragma unroll
        for (int i = 0; i < 8; ++i) rdA(smem + OFF_A0, fax, i & 3, i >> 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) rdB(smem + OFF_B0, fb0, i, 0);
        PIN();
        wait8(fax); wait4(fb0, 0);
        __builtin_amdgcn_s_barrier();
        PIN();
        for (int rel = 0; rel < ntile; ++rel) {
            char* const cur = smem + (rel & 1) * BUF_BYTES;
            char* const nxt = smem + ((rel & 1) ^ 1) * BUF_BYTES;
            // ---- Q0
            quadrant(0, 0, fax, fb0, [&](int i) {
                if (i < 4) rdB(cur + OFF_B0, fb0, i, 1);
                else if (i < 8) dmaA(0, cur, rel + 2, i - 4);
                else if (i == 15) { PIN(); wait4(fb0, 1); }
                else if (i >= 16 && i < 24) rdB(cur + OFF_B1, fb1, i & 3, (i - 16) >> 2);
            });
            rowsum(0, fax);
            PIN();
            wait8(fb1);
            PHASE_END();
            // ---- Q1
            quadrant(0, 1, fax, fb1, [&](int i) {
                if (i < 8) rdA(cur + OFF_A1, fay, i & 3, i >> 2);
                else if (i < 16 && !(i & 1)) dmaB(0, cur, rel + 2, (i - 8) >> 1);
            });
            PIN();
            wait8(fay);
            PHASE_END();
            // ---- Q2
            quadrant(1, 1, fay, fb1, [&](int i) {
                if (i < 4) rdA(nxt + OFF_A0, fax, i, 0);
                else if (i >= 8 && i < 16 && !(i & 1)) dmaB(1, cur, rel + 2, (i - 8) >> 1);
            });
            rowsum(1, fay);
            PIN();
            wait4(fax, 0);
            PHASE_END();
            // ---- Q3
            quadrant(1, 0, fay, fb0, [&](int i) {
                if (i < 4) rdA(nxt + OFF_A0, fax, i, 1);
                else if (i >= 8 && i < 16 && !(i & 1)) dmaA(1, cur, rel + 2, (i - 8) >> 1);
                else if (i >= 16 && i < 20) rdB(nxt + OFF_B0, fb0, i - 16, 0);
            });
            PIN();
            wait4(fax, 1); wait4(fb0, 0);
            PHASE_END();
        }
    }
    } else {
    if (ntile > 0) {
        // end of slot s: `tie` waits for the k-half(s) read in slot s - 1, which is at least 9 MFMAs behind by then; nfly > 0: a barrier
        // slot, what was issued more than nfly pieces ago has landed
#define SLOT_END(s, tie, nfly)                                                                                    \
    do {                                                                                                          \
        Q8_HS(1 + 2 * (s));                                                                                       \
        tie;                                                                                                      \
        PIN();                                                                                                    \
        if constexpr ((nfly) > 0) {                                                                               \
            Q8_HS(17 + 2 * ((s) >> 1));                                                                           \
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(nfly) : "memory");                                           \
            Q8_HS(18 + 2 * ((s) >> 1));                                                                           \
            __builtin_amdgcn_s_barrier();                                                                         \
            PIN();                                                                                                \
        }                                                                                                         \
        Q8_HS(2 + 2 * (s));                                                                                       \
    } while (0)
        // prologue = what the slots before K-tile 0 would have issued, in their order: A'0 B'0 B'1 A'1 of K-tiles 0 and 1; K-tile 0 has
        // landed, K-tile 1 stays in flight
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            char* const b = smem + t * BUF_BYTES;
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaA(0, b, t, i);
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaB(0, b, t, i);
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaB(1, b, t, i);
#pragma unroll
            for (int i = 0; i < 4; ++i) dmaA(1, b, t, i);
        }
        PIN();
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        PIN();
        // what the second half of a K-tile before the first would have read: A'0(0) and B'0(0); behind the barrier that follows, their
        // slots may be refilled
#pragma unroll
        for (int i = 0; i < 8; ++i) rdA(smem + OFF_A0, fax, i & 3, i >> 2);
#pragma unroll
        for (int i = 0; i < 8; ++i) rdB(smem + OFF_B0, fb0, i & 3, i >> 2);
        PIN();
        wait8(fax); wait8(fb0);
        __builtin_amdgcn_s_barrier();
        PIN();
        Q8_AT(1);
#ifdef Q8_STAMP
        st_[6] = __builtin_amdgcn_s_memrealtime();
#endif
        // the per-lane read addresses of the four A and B blocks in the K-tile's buffer (ad*) and in the other one (an*)
        uint32_t adA[4], adB[4], anA[4], anB[4];
        int adelta = BUF_BYTES;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            adA[i] = (uint32_t)(uintptr_t)LDS_PTR(smem) + trA[i];
            adB[i] = (uint32_t)(uintptr_t)LDS_PTR(smem) + trB[i];
            anA[i] = adA[i] + BUF_BYTES;
            anB[i] = adB[i] + BUF_BYTES;
        }
        // 16 MFMAs of a slot with `gap(integral_constant i)` behind MFMA i
        auto slot = [&](int mh, int nh, int kk, FragSet<true>& sa, FragSet<true>& sb, auto&& gap) __attribute__((always_inline)) {
            static_for<0, 16>([&](auto ic) __attribute__((always_inline)) {
                constexpr int i = decltype(ic)::value;
                mfma_acc(acc[mh * 4 + (i >> 2)][nh * 4 + (i & 3)], frag_of(sb.f[i & 3][kk]), frag_of(sa.f[i >> 2][kk]));
                gap(ic);
                PIN();
            });
        };
        for (int rel = 0; rel < ntile; ++rel) {
            char* const cur = smem + (rel & 1) * BUF_BYTES;
            char* const nxt = smem + ((rel & 1) ^ 1) * BUF_BYTES;
            Q8_HS(0);
            {
                // behind MFMA i of a slot: the read(s) the variadic part names for gap i, DMA pieces d0 / d1 behind MFMAs 9 / 13
#define GAP(d0, d1, ...)                                                                                          \
    [&](auto ic) __attribute__((always_inline)) {                                                                 \
        constexpr int i = decltype(ic)::value;                                                                    \
        LOOP_RD(__VA_ARGS__);                                                                                     \
        if constexpr (i == 9) LOOP_DMA(d0);                                                                       \
        if constexpr (i == 13) LOOP_DMA(d1);                                                                      \
    }
                slot(0, 0, 0, fax, fb0, GAP(dmaA(0, cur, rel + 2, 0), dmaA(0, cur, rel + 2, 1), if constexpr (i < 8) tr_read1<OFF_B1, 0, (i & 7)>(fb1, adB); else tr_read1<OFF_B1, 1, (i & 7)>(fb1, adB)));
                SLOT_END(0, (void)0, 0);
                slot(0, 0, 1, fax, fb0, GAP(dmaA(0, cur, rel + 2, 2), dmaA(0, cur, rel + 2, 3), if constexpr (i < 8) tr_read1<OFF_A1, 0, (i & 7)>(fay, adA)));
                rowsum(0, fax);
                SLOT_END(1, (wait4_older<8>(fb1, 0), wait4_older<8>(fb1, 1)), 0);
                slot(0, 1, 0, fax, fb1, GAP(dmaB(0, cur, rel + 2, 0), dmaB(0, cur, rel + 2, 1), if constexpr (i < 8) tr_read1<OFF_A1, 1, (i & 7)>(fay, adA)));
                SLOT_END(2, wait4_older<8>(fay, 0), 0);
                slot(0, 1, 1, fax, fb1, GAP(dmaB(0, cur, rel + 2, 2), dmaB(0, cur, rel + 2, 3), (void)0));
                SLOT_END(3, wait4(fay, 1), 16);
                slot(1, 0, 0, fay, fb0, GAP(dmaB(1, cur, rel + 2, 0), dmaB(1, cur, rel + 2, 1), if constexpr (i < 8) tr_read1<OFF_A0, 0, (i & 7)>(fax, anA)));
                SLOT_END(4, (void)0, 0);
                slot(1, 0, 1, fay, fb0, GAP(dmaB(1, cur, rel + 2, 2), dmaB(1, cur, rel + 2, 3), if constexpr (i < 8) tr_read1<OFF_A0, 1, (i & 7)>(fax, anA)));
                rowsum(1, fay);
                SLOT_END(5, wait4_older<8>(fax, 0), 0);
                slot(1, 1, 0, fay, fb1, GAP(dmaA(1, cur, rel + 2, 0), dmaA(1, cur, rel + 2, 1), if constexpr (i < 8) tr_read1<OFF_B0, 0, (i & 7)>(fb0, anB); else tr_read1<OFF_B0, 1, (i & 7)>(fb0, anB)));
                SLOT_END(6, wait4_older<15>(fax, 1), 0);
                // no reads in the last slot: the addresses change buffers here, two per gap
                slot(1, 1, 1, fay, fb1, [&](auto ic) __attribute__((always_inline)) {
                    constexpr int i = decltype(ic)::value;
                    if constexpr (i < 2) { adA[2 * i] += adelta; adA[2 * i + 1] += adelta; }
                    else if constexpr (i < 4) { adB[2 * i - 4] += adelta; adB[2 * i - 3] += adelta; }
                    else if constexpr (i < 6) { anA[2 * i - 8] -= adelta; anA[2 * i - 7] -= adelta; }
                    else if constexpr (i < 8) { anB[2 * i - 12] -= adelta; anB[2 * i - 11] -= adelta; }
                    if constexpr (i == 8) { adelta = -adelta; asm volatile("" : "+s"(adelta)); }
                    if constexpr (i == 9) LOOP_DMA(dmaA(1, cur, rel + 2, 2));
                    if constexpr (i == 13) LOOP_DMA(dmaA(1, cur, rel + 2, 3));
                });
                SLOT_END(7, wait8(fb0), 16);
#undef GAP
            }
        }
#undef SLOT_END
    }
    }
#ifdef Q8_STAMP
    st_[7] = __builtin_amdgcn_s_memrealtime();
#endif
    Q8_AT(2);
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_waitcnt vmcnt(0)" ::: "memory");     // the last MFMAs have written back; drain the look-ahead loads before LDS is reused
    PIN();
    __syncthreads();
    Q8_AT(3);
    if (do_rs && fg == 0) {     // racc[h][i][*] = sum_k A(m, k) for m = m0 + 128h + 64wm + 16(2wn + i) + fr
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + hh * 128 + wm * 64 + (2 * wn + i) * 16 + fr;
                if (m < p.M) {
                    if (p.kslices > 1) p.rowsum_ws[(int64_t)slice * p.M + m] = racc[hh][i][0];
                    else rowsum_store<T>(p, m, racc[hh][i][0]);
                }
            }
    }

    // ---- general epilogue: two passes (tile row halves mh) through LDS: 128 rows x 256 cols fp32 (swizzled 16-B chunks) ->
    // row-contiguous 16-byte bf16 stores.
    // acc[mh*4+mt][nh*4+nt][r] = C[mh*128 + wm*64 + mt*16 + fr][nh*128 + wn*64 + nt*16 + 4*fg + r]
    float* sC = (float*)smem;
    float* wsl = p.kslices > 1 ? p.ws + (int64_t)slice * p.M * p.N : nullptr;
    const f32x4_t bias0 = load_bias4<T>(p, n0 + (tid & 31) * 8), bias1 = load_bias4<T>(p, n0 + (tid & 31) * 8 + 4);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) __syncthreads();
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int ni = 0; ni < 8; ++ni) {
                const int ml = wm * 64 + mt * 16 + fr;                        // row inside this 128-row half
                const int ch = ((ni >> 2) * 32 + wn * 16 + (ni & 3) * 4 + fg) ^ (ml & 7);
                *(f32x4_t*)(sC + ml * 256 + ch * 4) = acc[pass * 4 + mt][ni];
            }
        __syncthreads();
#pragma unroll 2
        for (int it = 0; it < 16; ++it) {
            const int ml = it * 8 + (tid >> 5);
            const int c8 = tid & 31;                                   // 8 columns = fp32 chunks 2*c8, 2*c8+1
            const f32x4_t v0 = *(const f32x4_t*)(sC + ml * 256 + (((2 * c8) ^ (ml & 7)) << 2));
            const f32x4_t v1 = *(const f32x4_t*)(sC + ml * 256 + (((2 * c8 + 1) ^ (ml & 7)) << 2));
            const int m = m0 + pass * 128 + ml, n = n0 + c8 * 8;
            if (wsl) {
                splitk_store8(p, slice, m, n, v0, v1);
            } else {
                epilogue_store8<true, 0>(p, m, n, v0, v1, bias0, bias1);
            }
        }
#ifdef Q8_STAMP
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        st_[4 + pass] = __builtin_amdgcn_s_memtime();
#endif
    }
#ifdef Q8_STAMP
    if (lane == 0 && bid < Q8_STAMP_BLOCKS) {
        uint64_t* o = q8_stamp_buf + ((int64_t)bid * 4 + wave) * 64;
        for (int i = 0; i < 8; ++i) o[i] = st_[i];
        o[8] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_ID
        o[9] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // XCC_ID
        o[10] = ntile;
        o[11] = SLOTS;
        for (int i = 0; i < 32; ++i) o[16 + i] = hs_[i];
    }
#endif
#undef PHASE_END
#undef LOOP_DMA
#undef LOOP_RD
#undef PIN
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_8q_kernel(GemmArgs p) {
    gemm_8q_body<TA, TB>(p, blockIdx.x);
}
// valor_gemm_group: the weight gradients of a layer in one launch, each workgroup on the slot loop of its own problem
__global__ __launch_bounds__(256) void gemm_8q_kernel_grp(GemmGroupArgs a) {
    int i = 0;
    while (i + 1 < a.n && (int)blockIdx.x >= a.first[i + 1]) ++i;
    gemm_8q_body<true, true>(a.g[i], (int)blockIdx.x - a.first[i]);
}

void launch_gemm_8q(hipStream_t st, int transA, int transB, const GemmArgs& p_in) {
    GemmArgs p = p_in;
    p.fast_epi = 0;
    p.raster_g = 0;
    p.st_mode = 0;
    const int tiles = ((p.M + 255) / 256) * ((p.N + 255) / 256);
    dim3 grid(tiles * (p.kslices > 1 ? p.kslices : 1));
    const size_t lds = 2 * BUF_BYTES;
#define VALOR_8Q_LAUNCH(TA_, TB_)                                                                             \
    do {                                                                                                        \
        static bool attr_set = false;                                                                           \
        if (!attr_set) {                                                                                        \
            hipFuncSetAttribute((const void*)gemm_8q_kernel<TA_, TB_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            attr_set = true;                                                                                    \
        }                                                                                                       \
        hipLaunchKernelGGL((gemm_8q_kernel<TA_, TB_>), grid, dim3(256), lds, st, p);                            \
    } while (0)
    if (transA && transB) VALOR_8Q_LAUNCH(true, true);
    else if (!transA && !transB) VALOR_8Q_LAUNCH(false, false);
    else if (!transA && transB) VALOR_8Q_LAUNCH(false, true);
    else VALOR_8Q_LAUNCH(true, false);
#undef VALOR_8Q_LAUNCH
}

void launch_gemm_8q_group(hipStream_t st, const GemmGroupArgs& a) {
    const size_t lds = 2 * BUF_BYTES;
    static bool attr_set = false;
    if (!attr_set) {
        hipFuncSetAttribute((const void*)gemm_8q_kernel_grp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL(gemm_8q_kernel_grp, dim3(a.first[a.n]), dim3(256), lds, st, a);
}
