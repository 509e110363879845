// Retrieval search on an fp8 clip bank: the row quantiser and the scores-only fused token-pair kernel on the e4m3 matrix pipe.
//
// The law (search.quantize_rows_host restates it on the CPU, bit for bit): per token row x[0..D), all in fp32 round-to-nearest,
//     amax = max |x_d|;  amax < 2^-64: scale = 0, every code 0x00;  else scale = amax / 448, inv = 448 / amax,
//     code_d = e4m3fn(min(max(x_d * inv, -448), 448))          (OCP e4m3fn: RNE, subnormals and sign kept; the clamp keeps the convert
//                                                               inside the format's range, where no saturation rule is consulted)
// and the score of a (text, clip) pair is compute_fine_matrix_slice (pretrain.py:191-211) on the dequantised rows code * scale:
//     sim[a,b,t,v] = scaleA[a,t] scaleB[b,v] sum_d codeA codeB,  x = sim maskA maskB,  score = (sum_t wA max_v x + sum_v wB max_t x) / 2.
// fine_fused_fwd_fp8_kernel is fine_fused_fwd_kernel of contrastive_fused.hip (128 x 128 tile of token pairs, token axes padded to
// 16 / 32 / 64 slots, LDS-DMA into the XOR image of mma.h, out-of-range offsets read zeros, XCD remap, the A2B / B2A reductions in
// registers) with one change of operand: a 128-byte image row holds 128 codes, so a K step is 128 and a lane's 16-byte fragment feeds
// two v_mfma_f32_16x16x32_fp8_fp8 (its low and high 8 bytes; both operands use the same k order, so the contraction is exact).
// Products of two e4m3 values are exact in fp32; the only roundings are the fp32 accumulation and the scale multiply.
// Traffic per chunk: NB * Nv * (D + 4) bytes of bank instead of NB * Nv * D * 2.
#include "dpp.h"
#include "mma.h"

// ---------------------------------------------------------------------------------------------------------------- the quantiser
template <typename TT> DEVINL void load16(const TT* p, float (&f)[16]);
template <> DEVINL void load16<float>(const float* p, float (&f)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4_t v = *(const f32x4_t*)(p + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[4 * q + i] = v[i];
    }
}
template <> DEVINL void load16<bf16_t>(const bf16_t* p, float (&f)[16]) {
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

DEVINL float clamp448(float y) { return fminf(fmaxf(y, -448.f), 448.f); }
// four fp32 values in [-448, 448] -> four e4m3fn bytes, first value in the low byte (v_cvt_pk_fp8_f32: two values per instruction)
DEVINL uint32_t pack4_e4m3(float a, float b, float c, float d) {
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (uint32_t)v;
}

// one wave per row, four rows per workgroup; a lane owns 16 consecutive elements (16 output bytes) per pass. Rows of up to 1024
// elements stay in registers between the row maximum and the convert; longer rows are read a second time.
template <typename TT>
__global__ __launch_bounds__(256) void fp8_quantize_rows_kernel(const TT* __restrict__ x, int64_t ld, int64_t rows, int cols,
                                                               uint8_t* __restrict__ codes, float* __restrict__ scales) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const TT* xr = x + row * ld;
    uint8_t* cr = codes + row * cols;
    const int ng = cols >> 4;
    float f[16];
    float amax = 0.f;
    for (int g = lane; g < ng; g += 64) {
        load16<TT>(xr + g * 16, f);
#pragma unroll
        for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(f[i]));
    }
    amax = wave_max(amax);
    const bool live = amax >= 0x1p-64f;
    const float inv = live ? 448.f / amax : 0.f;
    if (lane == 0) scales[row] = live ? amax / 448.f : 0.f;
    for (int g = lane; g < ng; g += 64) {
        if (ng > 64) load16<TT>(xr + g * 16, f);
        u32x4_t o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = live ? pack4_e4m3(clamp448(f[4 * q] * inv), clamp448(f[4 * q + 1] * inv), clamp448(f[4 * q + 2] * inv),
                                     clamp448(f[4 * q + 3] * inv))
                        : 0u;
        *(u32x4_t*)(cr + g * 16) = o;
    }
}

// x: bf16 / fp32 [rows, ld], ld >= cols, cols % 16 == 0, rows 16-byte aligned; codes uint8 [rows, cols] dense; scales fp32 [rows]
extern "C" int valor_fp8_quantize_rows(void* stream, int dtype, const void* x, int64_t ld, int64_t rows, int cols, uint8_t* codes,
                                       float* scales) {
    if (rows == 0) return VALOR_OK;
    if (dtype != VALOR_DT_BF16 && dtype != VALOR_DT_F32) return VALOR_ERR_ARG;
    const int64_t esz = dtype == VALOR_DT_BF16 ? 2 : 4;
    if (rows < 0 || cols <= 0 || (cols % 16) != 0 || ld < cols || ((ld * esz) & 15) || !x || !codes || !scales) return VALOR_ERR_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)codes & 15) || ((uintptr_t)scales & 3)) return VALOR_ERR_ARG;
    const int64_t grid = (rows + 3) / 4;
    if (grid > 0x7fffffff) return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == VALOR_DT_BF16)
        hipLaunchKernelGGL((fp8_quantize_rows_kernel<bf16_t>), dim3((unsigned)grid), dim3(256), 0, st, (const bf16_t*)x, ld, rows, cols, codes, scales);
    else
        hipLaunchKernelGGL((fp8_quantize_rows_kernel<float>), dim3((unsigned)grid), dim3(256), 0, st, (const float*)x, ld, rows, cols, codes, scales);
    return valor_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- the score kernel
struct FineFp8Args {
    const void* ca; const void* cb;              // e4m3 codes [NA, T, D], [NB, Nv, D]
    const float* sA; const float* sB;            // row scales [NA, T], [NB, Nv]
    const float* maskA; const float* maskB;
    const float* wA; const float* wB;            // softmaxed token weights
    float* score;                                // [NA, NB]
    int NA, NB, T, Nv, D;
    uint32_t bytesA, bytesB;
};

#define FF8_OOB 0x7f000000       // a buffer offset past every operand: the range check returns zeros (padded token slots / tile tails)

typedef __attribute__((ext_vector_type(2))) long i64x2_t;

template <int TPB, int VPB>
__global__ __launch_bounds__(256, 2) void fine_fused_fwd_fp8_kernel(FineFp8Args p) {
    constexpr int BK = 128, IMG = 16384;
    constexpr int TP = 16 * TPB, VP = 16 * VPB;
    constexpr int RA = 128 / TP, CB = 128 / VP;          // texts / clips per workgroup tile
    constexpr int NPA = 4 / TPB, NPB = 4 / VPB;          // ... per 64 x 64 wave tile
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG];

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
    int voA[4], voB[4];
    {
        const int r = lane >> 3, c = (lane & 7) ^ r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = wave * 32 + j * 8 + r;                   // image row = tile row (A) / tile column (B)
            const int a = a0 + row / TP, t = row % TP;
            voA[j] = (a < p.NA && t < p.T) ? ((a * p.T + t) * p.D + c * 16) : FF8_OOB;
            const int b = b0 + row / VP, v = row % VP;
            voB[j] = (b < p.NB && v < p.Nv) ? ((b * p.Nv + v) * p.D + c * 16) : FF8_OOB;
        }
    }
    // one LDS stage, as in fine_fused_fwd_kernel: several workgroups per CU hide each other's loads
    const int nk = p.D / BK;
    for (int ks = 0; ks < nk; ++ks) {
        char* sA = smem + wave * 4096;
        char* sB = sA + IMG;
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(rsA, sA + j * 1024, voA[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(rsB, sB + j * 1024, voB[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) { voA[j] += BK; voB[j] += BK; }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* iA = smem;
        const char* iB = smem + IMG;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            // chunk kk * 4 + fg of a row: 16 codes; its low 8 bytes are this lane's k slice of one MFMA, its high 8 bytes of the next
            i64x2_t fn[4], fm[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fn[i] = *(const i64x2_t*)(iB + tile_off(wn * 64 + i * 16 + fr, kk * 4 + fg));
                fm[i] = *(const i64x2_t*)(iA + tile_off(wm * 64 + i * 16 + fr, kk * 4 + fg));
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
                        acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(fn[ni][h], fm[mi][h], acc[ni][mi], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- per-lane token constants. Row block mi: text ja = mi / TPB, token t = (mi % TPB) * 16 + fr; column block ni, r:
    // clip jb = ni / VPB, token v = (ni % VPB) * 16 + 4 * fg + r. The row scale rides on the mask: fA = scaleA maskA, fB = scaleB maskB.
    const float NEG = -INFINITY;
    float fAl[4], wAl[4], padT[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int a = a0 + wm * NPA + mi / TPB, t = (mi % TPB) * 16 + fr;
        const bool ok = a < p.NA && t < p.T;
        fAl[mi] = ok ? p.sA[a * p.T + t] * p.maskA[a * p.T + t] : 0.f;
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
            fBl[ni][r] = ok ? p.sB[b * p.Nv + v] * p.maskB[b * p.Nv + v] : 0.f;
            wBl[ni][r] = ok ? p.wB[b * p.Nv + v] : 0.f;
            padV[ni][r] = ok ? 0.f : NEG;
        }
    // x = S * (scaleA maskA * scaleB maskB), in place
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

// e4m3 codes with fp32 row scales, D % 128 == 0, T, Nv <= 64; scores only
extern "C" int valor_fine_fused_fwd_fp8(void* stream, const uint8_t* codesA, const float* scaleA, const uint8_t* codesB, const float* scaleB,
                                        const float* maskA, const float* maskB, const float* wA, const float* wB, float* score, int NA,
                                        int NB, int T, int Nv, int D) {
    if (NA == 0 || NB == 0) return VALOR_OK;
    if (NA < 0 || NB < 0 || T <= 0 || T > 64 || Nv <= 0 || Nv > 64 || D <= 0 || (D % 128) != 0) return VALOR_ERR_ARG;
    if (!codesA || !scaleA || !codesB || !scaleB || !maskA || !maskB || !wA || !wB || !score) return VALOR_ERR_ARG;
    if (((uintptr_t)codesA & 15) || ((uintptr_t)codesB & 15)) return VALOR_ERR_ARG;
    const int64_t bytesA = (int64_t)NA * T * D, bytesB = (int64_t)NB * Nv * D;
    if (bytesA >= FF8_OOB || bytesB >= FF8_OOB) return VALOR_ERR_ARG;
    FineFp8Args p;
    p.ca = codesA; p.cb = codesB; p.sA = scaleA; p.sB = scaleB; p.maskA = maskA; p.maskB = maskB; p.wA = wA; p.wB = wB; p.score = score;
    p.NA = NA; p.NB = NB; p.T = T; p.Nv = Nv; p.D = D; p.bytesA = (uint32_t)bytesA; p.bytesB = (uint32_t)bytesB;
    const int tpb = T <= 16 ? 1 : (T <= 32 ? 2 : 4), vpb = Nv <= 16 ? 1 : (Nv <= 32 ? 2 : 4);
    const int RA = 8 / tpb, CB = 8 / vpb;
    const int64_t grid = (int64_t)((NA + RA - 1) / RA) * ((NB + CB - 1) / CB);
    if (grid > 0x7fffffff) return VALOR_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
#define FF8_LAUNCH(TPB_, VPB_) hipLaunchKernelGGL((fine_fused_fwd_fp8_kernel<TPB_, VPB_>), dim3((unsigned)grid), dim3(256), 0, st, p)
    switch (tpb * 8 + vpb) {
        case 1 * 8 + 1: FF8_LAUNCH(1, 1); break;
        case 1 * 8 + 2: FF8_LAUNCH(1, 2); break;
        case 1 * 8 + 4: FF8_LAUNCH(1, 4); break;
        case 2 * 8 + 1: FF8_LAUNCH(2, 1); break;
        case 2 * 8 + 2: FF8_LAUNCH(2, 2); break;
        case 2 * 8 + 4: FF8_LAUNCH(2, 4); break;
        case 4 * 8 + 1: FF8_LAUNCH(4, 1); break;
        case 4 * 8 + 2: FF8_LAUNCH(4, 2); break;
        default: FF8_LAUNCH(4, 4); break;
    }
#undef FF8_LAUNCH
    return valor_launch_status();
}
