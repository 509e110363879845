// Retrieval search on an MXFP4 clip bank: the OCP MX row quantiser and the scores-only fused token-pair kernel on the block-scaled
// matrix pipe (v_mfma_scale_f32_16x16x128_f8f6f4: MX-e4m3 query rows against MX-e2m1 bank rows).
//
// The quantiser's law (search.mx_quantize_rows_host restates it on the CPU, bit for bit) is the OCP MX v1.0 conversion, per block of 32
// consecutive elements of a row:
//     amax = max |x|;  e = floor(log2 amax) (the fp32 exponent field - 127; a zero or subnormal amax counts as e = -127)
//     s = clamp(e - emax, -127, 127), emax = 8 (e4m3) / 2 (e2m1);  scale byte = s + 127 (0 .. 254, never 255)
//     code = RNE(clamp(x * 2^-s, -max, max)), max = 448 / 6; the multiply by a power of two is exact, ties go to the even code, the sign
//     of zero and the element format's subnormals are kept. An all-zero block has scale byte 0 and zero codes.
//     e2m1: element 2i in the low nibble of byte i, element 2i + 1 in the high nibble.
// The score of a (text, clip) pair is compute_fine_matrix_slice (pretrain.py:191-211) on the dequantised rows code * 2^(byte - 127):
//     sim[a,b,t,v] = sum_d deqA deqB,  x = sim maskA maskB,  score = (sum_t wA max_v x + sum_v wB max_t x) / 2.
// fine_fused_fwd_mx_kernel is fine_fused_fwd_fp8_kernel of search_fp8.hip (128 x 128 tile of token pairs, token axes padded to 16 / 32 /
// 64 slots, LDS-DMA staging, out-of-range offsets read zeros, XCD remap, the A2B / B2A reductions in registers) with another operand:
// a K step is 128 elements, 128 bytes of a query row (the XOR image of mma.h) and 64 bytes of a bank row (a 64-byte-row image, below),
// and one scaled MFMA per 16 x 16 block consumes it. The operand map, as the exact test of tests/test_search_mx_gpu.py pinned it on
// the device (g = l >> 4, operand row l & 15):
//     e2m1 (16 bytes, the low 4 of 8 dwords): the 32 elements k = 32 g .. + 31, one MX block, element 2i in the low nibble of byte i;
//     e4m3 (32 bytes, 8 dwords): dwords 0-3 are k = 16 g .. + 15 and dwords 4-7 are k = 64 + 16 g .. + 15 -- two half blocks, NOT
//     the lane's own block (the 8-bit form is laid out as two K = 64 halves);
//     scales: lane (row, g) supplies the E8M0 byte of block g (k = 32 g .. + 31) of its row, for either format, in byte 0 of its
//     scale register (op_sel 0).
// The hardware applies both scales; the epilogue only masks.
// The bank rows are the MFMA's FIRST operand (cbsz = e2m1) and the query rows its second (blgp = e4m3), as in the fp8 kernel, so the
// accumulator layout and the whole epilogue are that kernel's.
// Products of an e4m3 and an e2m1 value and the power-of-two scales are exact in fp32; the only roundings are the accumulation's.
// Traffic per chunk: NB * Nv * (D / 2 + D / 32 + 4) bytes of bank (codes, scale bytes, fp32 token weights).
#include "dpp.h"
#include "mma.h"

// ---------------------------------------------------------------------------------------------------------------- the quantiser
template <typename TT> DEVINL void mx_load16(const TT* p, float (&f)[16]);
template <> DEVINL void mx_load16<float>(const float* p, float (&f)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4_t v = *(const f32x4_t*)(p + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[4 * q + i] = v[i];
    }
}
template <> DEVINL void mx_load16<bf16_t>(const bf16_t* p, float (&f)[16]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const u32x4_t v = *(const u32x4_t*)(p + 8 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[8 * q + 2 * i] = __uint_as_float(v[i] << 16);
            f[8 * q + 2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
        }
    }
}

// four fp32 values in [-448, 448] -> four e4m3fn bytes, first value in the low byte (v_cvt_pk_fp8_f32: RNE, subnormals and sign kept)
DEVINL uint32_t mx_pack4_e4m3(float a, float b, float c, float d) {
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (uint32_t)v;
}
// one fp32 value -> its e2m1 nibble. The magnitudes are 0, .5, 1, 1.5, 2, 3, 4, 6 (codes 0 .. 7): seven compares at the midpoints,
// `>` where the lower neighbour has the even code and `>=` where the upper one has; anything above 5 is 6 (the clamp).
DEVINL uint32_t mx_e2m1(float y) {
    const float m = fabsf(y);
    const uint32_t c = (uint32_t)(m > 0.25f) + (uint32_t)(m >= 0.75f) + (uint32_t)(m > 1.25f) + (uint32_t)(m >= 1.75f) + (uint32_t)(m > 2.5f) +
                       (uint32_t)(m >= 3.5f) + (uint32_t)(m > 5.0f);
    return c | ((__float_as_uint(y) >> 28) & 8u);
}

// a lane owns 16 consecutive elements of a row, two neighbouring lanes one block of 32. Rows are independent of the launch shape.
template <typename TT, int FMT>
__global__ __launch_bounds__(256) void mx_quantize_rows_kernel(const TT* __restrict__ x, int64_t ld, int64_t rows, int cols,
                                                              uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
    const int ng = cols >> 4;                                  // even: cols % 32 == 0
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows * ng) return;                              // the two lanes of a block leave together
    const int64_t row = gid / ng;
    const int g = (int)(gid - row * ng);
    float f[16];
    mx_load16<TT>(x + row * ld + (int64_t)g * 16, f);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(f[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    constexpr int EMAX = FMT == VALOR_MX_E2M1 ? 2 : 8;
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127;
    const int s = max(e - EMAX, -127);
    const float mul = __uint_as_float((uint32_t)(127 - s) << 23);          // 2^-s: 127 - s is in [2, 254]
    if ((g & 1) == 0) scales[row * (cols >> 5) + (g >> 1)] = (uint8_t)(s + 127);
    if constexpr (FMT == VALOR_MX_E2M1) {
        u32x2_t o;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) w |= mx_e2m1(f[8 * q + i] * mul) << (4 * i);
            o[q] = w;
        }
        *(u32x2_t*)(codes + row * (cols >> 1) + (int64_t)g * 8) = o;
    } else {
        u32x4_t o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = fminf(fmaxf(f[4 * q + i] * mul, -448.f), 448.f);
            o[q] = mx_pack4_e4m3(y[0], y[1], y[2], y[3]);
        }
        *(u32x4_t*)(codes + row * cols + (int64_t)g * 16) = o;
    }
}

// x: bf16 / fp32 [rows, ld], ld >= cols, cols % 32 == 0, rows 16-byte aligned; codes uint8 [rows, cols] (e4m3) / [rows, cols / 2] (e2m1),
// dense, 16-byte aligned; scales uint8 [rows, cols / 32]
extern "C" int valor_mx_quantize_rows(void* stream, int dtype, const void* x, int64_t ld, int64_t rows, int cols, int fmt, uint8_t* codes,
                                      uint8_t* scales) {
    if (rows == 0) return VALOR_OK;
    if (dtype != VALOR_DT_BF16 && dtype != VALOR_DT_F32) return VALOR_ERR_ARG;
    if (fmt != VALOR_MX_E4M3 && fmt != VALOR_MX_E2M1) return VALOR_ERR_ARG;
    const int64_t esz = dtype == VALOR_DT_BF16 ? 2 : 4;
    if (rows < 0 || cols <= 0 || (cols % 32) != 0 || ld < cols || ((ld * esz) & 15) || !x || !codes || !scales) return VALOR_ERR_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)codes & 15)) return VALOR_ERR_ARG;
    if (rows > (int64_t)0x7fffffff * 16) return VALOR_ERR_ARG;
    const int64_t grid = (rows * (cols >> 4) + 255) / 256;
    if (grid > 0x7fffffff) return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
#define MXQ_LAUNCH(TT_, FMT_) \
    hipLaunchKernelGGL((mx_quantize_rows_kernel<TT_, FMT_>), dim3((unsigned)grid), dim3(256), 0, st, (const TT_*)x, ld, rows, cols, codes, scales)
    if (dtype == VALOR_DT_BF16) {
        if (fmt == VALOR_MX_E2M1) MXQ_LAUNCH(bf16_t, VALOR_MX_E2M1); else MXQ_LAUNCH(bf16_t, VALOR_MX_E4M3);
    } else {
        if (fmt == VALOR_MX_E2M1) MXQ_LAUNCH(float, VALOR_MX_E2M1); else MXQ_LAUNCH(float, VALOR_MX_E4M3);
    }
#undef MXQ_LAUNCH
    return valor_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- the score kernel
struct FineMxArgs {
    const void* ca; const void* cb;              // MX-e4m3 codes [NA, T, D], MX-e2m1 codes [NB, Nv, D / 2]
    const void* sA; const void* sB;              // E8M0 scale bytes [NA, T, D / 32], [NB, Nv, D / 32]
    const float* maskA; const float* maskB;
    const float* wA; const float* wB;            // softmaxed token weights
    float* score;                                // [NA, NB]
    int NA, NB, T, Nv, D;
    uint32_t bytesA, bytesB, bytesSA, bytesSB;
};

#define FMX_OOB 0x7f000000       // a buffer offset past every operand: the range check returns zeros (padded token slots / tile tails)

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(8))) int i32x8_t;

// the bank image: 128 rows of 64 bytes (4 chunks of 16 B = one MX block each); chunk c of row r lives at r * 64 + ((c ^ ((r >> 2) & 3)) << 4),
// so the 16 rows a ds_read_b128 group reads (one chunk index) fall into 16 distinct 16-byte slots of a 256-byte bank line
DEVINL int mx_bank_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

template <int TPB, int VPB>
__global__ __launch_bounds__(256, 2) void fine_fused_fwd_mx_kernel(FineMxArgs p) {
    constexpr int IMGA = 16384, IMGB = 8192;
    constexpr int TP = 16 * TPB, VP = 16 * VPB;
    constexpr int RA = 128 / TP, CB = 128 / VP;          // texts / clips per workgroup tile
    constexpr int NPA = 4 / TPB, NPB = 4 / VPB;          // ... per 64 x 64 wave tile
    __shared__ __attribute__((aligned(16))) char smem[IMGA + IMGB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;

    const int tiles_b = (p.NB + CB - 1) / CB, tiles_a = (p.NA + RA - 1) / RA;
    const int logical = xcd_remap(blockIdx.x, tiles_a * tiles_b);
    const int ta = logical / tiles_b, tb = logical - ta * tiles_b;
    const int a0 = ta * RA, b0 = tb * CB;

    f32x4_t acc[4][4];      // [ni][mi]: S[row = wm*64 + mi*16 + fr][col = wn*64 + ni*16 + 4*fg + r]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const rsrc_t rsA = make_rsrc(p.ca, p.bytesA), rsB = make_rsrc(p.cb, p.bytesB);
    const rsrc_t rsSA = make_rsrc(p.sA, p.bytesSA), rsSB = make_rsrc(p.sB, p.bytesSB);
    const int DB = p.D >> 1, DS = p.D >> 5;              // bytes of a bank row's codes, of a row's scale bytes (a multiple of 4)
    int voA[4], voB[2];
    {
        const int r = lane >> 3, c = (lane & 7) ^ r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = wave * 32 + j * 8 + r;                   // query image row = tile row
            const int a = a0 + row / TP, t = row % TP;
            voA[j] = (a < p.NA && t < p.T) ? ((a * p.T + t) * p.D + c * 16) : FMX_OOB;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = wave * 32 + j * 16 + (lane >> 2);        // bank image row = tile column
            const int c = (lane & 3) ^ ((row >> 2) & 3);
            const int b = b0 + row / VP, v = row % VP;
            voB[j] = (b < p.NB && v < p.Nv) ? ((b * p.Nv + v) * DB + c * 16) : FMX_OOB;
        }
    }
    // the dword of scale bytes of this lane's operand rows for the current K step: byte fg of it is the lane's own block
    int soA[4], soB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rowa = wm * 64 + i * 16 + fr, a = a0 + rowa / TP, t = rowa % TP;
        soA[i] = (a < p.NA && t < p.T) ? (a * p.T + t) * DS : FMX_OOB;
        const int rowb = wn * 64 + i * 16 + fr, b = b0 + rowb / VP, v = rowb % VP;
        soB[i] = (b < p.NB && v < p.Nv) ? (b * p.Nv + v) * DS : FMX_OOB;
    }
    // one LDS stage, as in fine_fused_fwd_kernel: several workgroups per CU hide each other's loads
    const int nk = p.D / 128;
    for (int ks = 0; ks < nk; ++ks) {
        int scA[4], scB[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            scA[i] = __builtin_amdgcn_raw_buffer_load_b32(rsSA, soA[i], 0, 0);
            scB[i] = __builtin_amdgcn_raw_buffer_load_b32(rsSB, soB[i], 0, 0);
            soA[i] += 4; soB[i] += 4;
        }
        char* sA = smem + wave * 4096;
        char* sB = smem + IMGA + wave * 2048;
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(rsA, sA + j * 1024, voA[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(rsB, sB + j * 1024, voB[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) voA[j] += 128;
#pragma unroll
        for (int j = 0; j < 2; ++j) voB[j] += 64;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* iA = smem;
        const char* iB = smem + IMGA;
        i32x8_t fn[4], fm[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const i32x4_t bq = *(const i32x4_t*)(iB + mx_bank_off(wn * 64 + i * 16 + fr, fg));
            // an 8-bit operand's dwords 0-3 are k = 16 fg .. + 15 and its dwords 4-7 are k = 64 + 16 fg .. + 15 (chunks fg and 4 + fg)
            const i32x4_t lo = *(const i32x4_t*)(iA + tile_off(wm * 64 + i * 16 + fr, fg));
            const i32x4_t hi = *(const i32x4_t*)(iA + tile_off(wm * 64 + i * 16 + fr, 4 + fg));
            fn[i] = (i32x8_t){bq[0], bq[1], bq[2], bq[3], 0, 0, 0, 0};
            fm[i] = (i32x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            scA[i] = (int)(((uint32_t)scA[i] >> (8 * fg)) & 0xffu);
            scB[i] = (int)(((uint32_t)scB[i] >> (8 * fg)) & 0xffu);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fn[ni], fm[mi], acc[ni][mi], VALOR_MX_E2M1, VALOR_MX_E4M3, 0,
                                                                               scB[ni], 0, scA[mi]);
        __syncthreads();
    }

    // ---- per-lane token constants. Row block mi: text ja = mi / TPB, token t = (mi % TPB) * 16 + fr; column block ni, r:
    // clip jb = ni / VPB, token v = (ni % VPB) * 16 + 4 * fg + r. The scales are applied already: fA = maskA, fB = maskB.
    const float NEG = -INFINITY;
    float fAl[4], wAl[4], padT[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int a = a0 + wm * NPA + mi / TPB, t = (mi % TPB) * 16 + fr;
        const bool ok = a < p.NA && t < p.T;
        fAl[mi] = ok ? p.maskA[a * p.T + t] : 0.f;
        wAl[mi] = ok ? p.wA[a * p.T + t] : 0.f;
        padT[mi] = ok ? 0.f : NEG;
    }
    float fBl[4][4], wBl[4][4], padV[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + wn * NPB + ni / VPB, v = (ni % VPB) * 16 + 4 * fg + r;
            const bool ok = b < p.NB && v < p.Nv;
            fBl[ni][r] = ok ? p.maskB[b * p.Nv + v] : 0.f;
            wBl[ni][r] = ok ? p.wB[b * p.Nv + v] : 0.f;
            padV[ni][r] = ok ? 0.f : NEG;
        }
    // x = S * (maskA * maskB), in place
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ni][mi][r] = acc[ni][mi][r] * (fAl[mi] * fBl[ni][r]);

    float ps[NPA][NPB];       // per-lane partial of 2 * score of every (text, clip) pair of this wave tile
#pragma unroll
    for (int i = 0; i < NPA; ++i)
#pragma unroll
        for (int j = 0; j < NPB; ++j) ps[i][j] = 0.f;

    // ---- A2B: max over the clip's tokens for every text token. In-lane over (column block, r), then the 4 lane groups fg that hold
    // the other v of the same t (lanes fr, fr + 16, fr + 32, fr + 48).
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int jb = 0; jb < NPB; ++jb) {
            float best = NEG;
#pragma unroll
            for (int q = 0; q < VPB; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) best = fmaxf(best, acc[jb * VPB + q][mi][r] + padV[jb * VPB + q][r]);
            float mx = fmaxf(best, __shfl_xor(best, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (fg == 0) ps[mi / TPB][jb] += mx * wAl[mi];        // counted once per t (all four lane groups hold the same value)
        }
    // ---- B2A: max over the text's tokens for every clip token. In-lane over the row blocks of one text, then the 16 lanes fr of
    // the DPP row.
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int ja = 0; ja < NPA; ++ja) {
            const int jb = ni / VPB;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float best = NEG;
#pragma unroll
                for (int q = 0; q < TPB; ++q) best = fmaxf(best, acc[ni][ja * TPB + q][r] + padT[ja * TPB + q]);
                const float mx = row16_max(best);
                if (fr == 0) ps[ja][jb] += (wBl[ni][r] != 0.f) ? mx * wBl[ni][r] : 0.f;      // padded / masked slots: weight 0 (and mx may be -inf)
            }
        }
    // ---- score = half the sum over the wave's lanes
#pragma unroll
    for (int ja = 0; ja < NPA; ++ja)
#pragma unroll
        for (int jb = 0; jb < NPB; ++jb) {
            float s = row16_sum(ps[ja][jb]);
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            const int a = a0 + wm * NPA + ja, b = b0 + wn * NPB + jb;
            if (lane == 0 && a < p.NA && b < p.NB) p.score[(int64_t)a * p.NB + b] = 0.5f * s;
        }
}

// MX-e4m3 query rows against MX-e2m1 bank rows, D % 128 == 0, T, Nv <= 64; scores only
extern "C" int valor_fine_fused_fwd_mx(void* stream, const uint8_t* codesA, const uint8_t* scaleA, const uint8_t* codesB, const uint8_t* scaleB,
                                       const float* maskA, const float* maskB, const float* wA, const float* wB, float* score, int NA,
                                       int NB, int T, int Nv, int D) {
    if (NA == 0 || NB == 0) return VALOR_OK;
    if (NA < 0 || NB < 0 || T <= 0 || T > 64 || Nv <= 0 || Nv > 64 || D <= 0 || (D % 128) != 0) return VALOR_ERR_ARG;
    if (!codesA || !scaleA || !codesB || !scaleB || !maskA || !maskB || !wA || !wB || !score) return VALOR_ERR_ARG;
    if (((uintptr_t)codesA & 15) || ((uintptr_t)codesB & 15) || ((uintptr_t)scaleA & 3) || ((uintptr_t)scaleB & 3)) return VALOR_ERR_ARG;
    const int64_t bytesA = (int64_t)NA * T * D, bytesB = (int64_t)NB * Nv * (D / 2);
    if (bytesA >= FMX_OOB || bytesB >= FMX_OOB) return VALOR_ERR_ARG;
    FineMxArgs p;
    p.ca = codesA; p.cb = codesB; p.sA = scaleA; p.sB = scaleB; p.maskA = maskA; p.maskB = maskB; p.wA = wA; p.wB = wB; p.score = score;
    p.NA = NA; p.NB = NB; p.T = T; p.Nv = Nv; p.D = D; p.bytesA = (uint32_t)bytesA; p.bytesB = (uint32_t)bytesB;
    p.bytesSA = (uint32_t)(bytesA / 32); p.bytesSB = (uint32_t)(bytesB / 16);
    const int tpb = T <= 16 ? 1 : (T <= 32 ? 2 : 4), vpb = Nv <= 16 ? 1 : (Nv <= 32 ? 2 : 4);
    const int RA = 8 / tpb, CB = 8 / vpb;
    const int64_t grid = (int64_t)((NA + RA - 1) / RA) * ((NB + CB - 1) / CB);
    if (grid > 0x7fffffff) return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
#define FMX_LAUNCH(TPB_, VPB_) hipLaunchKernelGGL((fine_fused_fwd_mx_kernel<TPB_, VPB_>), dim3((unsigned)grid), dim3(256), 0, st, p)
    switch (tpb * 8 + vpb) {
        case 1 * 8 + 1: FMX_LAUNCH(1, 1); break;
        case 1 * 8 + 2: FMX_LAUNCH(1, 2); break;
        case 1 * 8 + 4: FMX_LAUNCH(1, 4); break;
        case 2 * 8 + 1: FMX_LAUNCH(2, 1); break;
        case 2 * 8 + 2: FMX_LAUNCH(2, 2); break;
        case 2 * 8 + 4: FMX_LAUNCH(2, 4); break;
        case 4 * 8 + 1: FMX_LAUNCH(4, 1); break;
        case 4 * 8 + 2: FMX_LAUNCH(4, 2); break;
        default: FMX_LAUNCH(4, 4); break;
    }
#undef FMX_LAUNCH
    return valor_launch_status();
}
