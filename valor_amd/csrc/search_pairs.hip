// Retrieval search, pair scores: every query against ITS OWN list of clips, read by index from a feature store (the second stage of a
// two-stage search on an fp8 bank, and the search within a given subset of the gallery).
//
// The law is that of fine_fused_fwd_kernel (contrastive_fused.hip) in its scores-only mode, for the pair (a, b = cand[a, c]):
//     x[t,v] = S[t,v] * maskA[a,t]                                      (the clip mask is all ones and implicit)
//     score  = (sum_t wA[a,t] max_v x + sum_v wB[b,v] max_t x) / 2      pretrain.py:191-211
// with the token axes padded to TP = 16 * TPB and VP = 16 * VPB slots: a padded slot holds S = 0, is excluded from the maxima (-inf
// added) and carries weight 0. A candidate outside [0, NS) is never dereferenced: its score is -inf.
//
// Shape: a workgroup owns one query and PAIR_BLOCK consecutive candidates of its list. The query's token rows go to LDS once, as one
// XOR image of mma.h (TP rows x 128 bytes) per 64-deep K step; each of the four waves then takes candidates in turn. A wave reads the
// clip's fragments straight from the store into registers (lane (fr, fg) = the 16 bytes of token row 16 q + fr at k chunk fg: the
// fragment layout itself, 64 contiguous bytes per row and load, the two loads of a K step cover the 128-byte line) through a buffer
// resource that spans exactly this clip, so the padded token rows read zeros from the range check. One step of look-ahead on those
// loads; other workgroups on the CU hide the rest. The accumulators are acc[VPB][TPB] 16 x 16 tiles in the orientation of the fused
// kernel (row 4 fg + r = clip token, column fr = text token) and are reduced in its order: A2B in-lane then across the four lane
// groups, B2A in-lane then across the DPP row, the weighted partial sums by row16_sum and two shuffles.
// A query image larger than 64 KiB of LDS (D > 32768 / TP) is staged in segments along D; the workgroup then restages per round of
// four candidates.
#include "dpp.h"
#include "mma.h"

#define PAIR_BLOCK 16            // candidates per workgroup: four rounds of one candidate per wave
#define PAIR_OOB 0x7f000000      // a buffer offset past every clip: the range check returns zeros (padded token slots)
#define PAIR_LDS_BYTES 65536

struct PairArgs {
    const bf16_t* fa;            // [NA, T, D]
    const float* maskA; const float* wA;
    const char* store;           // bf16 [NS, Nv, D]
    const float* wStore;         // [NS, Nv]
    const int64_t* cand; int64_t ld_cand;
    float* score; int64_t ld_score;
    int64_t NS;
    int NA, C, T, Nv, D;
    int seg;                     // elements of D per LDS segment (a multiple of 64)
};

template <int TPB, int VPB>
__global__ __launch_bounds__(256) void fine_score_pairs_kernel(PairArgs p) {
    typedef bf16_t T;
    constexpr int TP = 16 * TPB;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int nblk = (p.C + PAIR_BLOCK - 1) / PAIR_BLOCK;
    const int a = blockIdx.x / nblk;
    const int c0 = (blockIdx.x - a * nblk) * PAIR_BLOCK;
    const int nc = min(PAIR_BLOCK, p.C - c0);
    const int rounds = (nc + 3) >> 2;
    const int nseg = (p.D + p.seg - 1) / p.seg;
    const float NEG = -INFINITY;

    // ---- per-lane token constants of the query: block mi, token t = mi * 16 + fr
    float mAl[TPB], wAl[TPB], padT[TPB];
#pragma unroll
    for (int mi = 0; mi < TPB; ++mi) {
        const int t = mi * 16 + fr;
        const bool ok = t < p.T;
        mAl[mi] = ok ? p.maskA[a * p.T + t] : 0.f;
        wAl[mi] = ok ? p.wA[a * p.T + t] : 0.f;
        padT[mi] = ok ? 0.f : NEG;
    }
    // clip side: block q, token v = q * 16 + 4 * fg + r (epilogue) and the fragment row q * 16 + fr (loads)
    int voB[VPB];
#pragma unroll
    for (int q = 0; q < VPB; ++q) {
        const int v = q * 16 + fr;
        voB[q] = v < p.Nv ? (v * p.D + fg * 8) * 2 : PAIR_OOB;
    }
    const uint32_t clip_bytes = (uint32_t)p.Nv * p.D * 2;

    for (int rnd = 0; rnd < rounds; ++rnd) {
        const int c = c0 + rnd * 4 + wave;
        const bool valid = c < p.C;                                   // wave-uniform
        int64_t b = -1;
        if (valid) b = p.cand[(int64_t)a * p.ld_cand + c];
        const bool live = valid && b >= 0 && b < p.NS;               // only then is the store touched
        const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)b), bhi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)b >> 32));
        const int64_t bu = (int64_t)(((uint64_t)bhi << 32) | blo);
        const rsrc_t rs = make_rsrc(p.store + (live ? bu : (int64_t)0) * (int64_t)clip_bytes, live ? clip_bytes : 0u);

        f32x4_t acc[VPB][TPB];    // S[clip token q*16 + 4*fg + r][text token mi*16 + fr]
#pragma unroll
        for (int q = 0; q < VPB; ++q)
#pragma unroll
            for (int mi = 0; mi < TPB; ++mi) acc[q][mi] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

        for (int sg = 0; sg < nseg; ++sg) {
            const int d0 = sg * p.seg, dn = min(p.seg, p.D - d0);
            if (nseg > 1 || rnd == 0) {                               // workgroup-uniform: the query image (a segment of it)
                if (rnd | sg) __syncthreads();
                const int chunks = TP * (dn >> 3);
                for (int i = tid; i < chunks; i += 256) {
                    const int ks = i / (TP * 8), rem = i - ks * (TP * 8), row = rem >> 3, ch = rem & 7;
                    u32x4_t v = (u32x4_t){0u, 0u, 0u, 0u};
                    if (row < p.T) v = *(const u32x4_t*)(p.fa + ((int64_t)a * p.T + row) * p.D + d0 + ks * 64 + ch * 8);
                    *(u32x4_t*)(smem + ks * (TP * TILE_ROW_BYTES) + tile_off(row, ch)) = v;
                }
                __syncthreads();
            }
            if (!live) continue;
            const int steps = dn >> 5;                                // 32 k per step: image ks = s >> 1, chunk group kk = s & 1
            u32x4_t nxt[VPB];
#pragma unroll
            for (int q = 0; q < VPB; ++q) nxt[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, voB[q] + d0 * 2, 0, 0);
            for (int s = 0; s < steps; ++s) {
                bf16x8_t fn[VPB], fm[TPB];
#pragma unroll
                for (int q = 0; q < VPB; ++q) fn[q] = __builtin_bit_cast(bf16x8_t, nxt[q]);
                if (s + 1 < steps) {
#pragma unroll
                    for (int q = 0; q < VPB; ++q) nxt[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, voB[q] + (d0 + (s + 1) * 32) * 2, 0, 0);
                }
                const char* img = smem + (s >> 1) * (TP * TILE_ROW_BYTES);
#pragma unroll
                for (int mi = 0; mi < TPB; ++mi) fm[mi] = read_frag<T>(img, mi * 16 + fr, (s & 1) * 4 + fg);
#pragma unroll
                for (int q = 0; q < VPB; ++q)
#pragma unroll
                    for (int mi = 0; mi < TPB; ++mi) acc[q][mi] = Mma<T>::mma(fn[q], fm[mi], acc[q][mi]);
            }
        }
        if (!valid) continue;
        if (!live) {
            if (lane == 0) p.score[(int64_t)a * p.ld_score + c] = NEG;
            continue;
        }

        float wBl[VPB][4], padV[VPB][4];
#pragma unroll
        for (int q = 0; q < VPB; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = q * 16 + 4 * fg + r;
                const bool ok = v < p.Nv;
                wBl[q][r] = ok ? p.wStore[bu * p.Nv + v] : 0.f;
                padV[q][r] = ok ? 0.f : NEG;
            }
        // x = (S * maskA) * maskB with maskB = 1 on the clip's tokens (a padded slot holds S = 0)
#pragma unroll
        for (int q = 0; q < VPB; ++q)
#pragma unroll
            for (int mi = 0; mi < TPB; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[q][mi][r] = acc[q][mi][r] * mAl[mi];

        float ps = 0.f;           // per-lane partial of 2 * score
        // ---- A2B: max over the clip's tokens for every text token: in-lane over (q, r), then the four lane groups fg
#pragma unroll
        for (int mi = 0; mi < TPB; ++mi) {
            float best = NEG;
#pragma unroll
            for (int q = 0; q < VPB; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) best = fmaxf(best, acc[q][mi][r] + padV[q][r]);
            float mx = fmaxf(best, __shfl_xor(best, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (fg == 0) ps += mx * wAl[mi];                          // counted once per t
        }
        // ---- B2A: max over the text's tokens for every clip token: in-lane over the row blocks, then the 16 lanes of the DPP row
#pragma unroll
        for (int q = 0; q < VPB; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float best = NEG;
#pragma unroll
                for (int mi = 0; mi < TPB; ++mi) best = fmaxf(best, acc[q][mi][r] + padT[mi]);
                const float mx = row16_max(best);
                if (fr == 0) ps += (wBl[q][r] != 0.f) ? mx * wBl[q][r] : 0.f;      // padded slots: weight 0 (and mx may be -inf)
            }
        float s = row16_sum(ps);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (lane == 0) p.score[(int64_t)a * p.ld_score + c] = 0.5f * s;
    }
}

// featA bf16 [NA, T, D]; storeB bf16 [NS, Nv, D] with wStoreB fp32 [NS, Nv]; cand int64 [NA, ld_cand]; score fp32 [NA, ld_score]
extern "C" int valor_fine_score_pairs(void* stream, const void* featA, const float* maskA, const float* wA, const void* storeB,
                                      const float* wStoreB, int64_t NS, const int64_t* cand, int64_t ld_cand, float* score,
                                      int64_t ld_score, int NA, int C, int T, int Nv, int D) {
    if (NA == 0 || C == 0) return VALOR_OK;
    if (NA < 0 || C < 0 || NS < 0 || T <= 0 || T > 64 || Nv <= 0 || Nv > 64 || D <= 0 || (D % 64) != 0) return VALOR_ERR_ARG;
    if (!featA || !maskA || !wA || !storeB || !wStoreB || !cand || !score || ld_cand < C || ld_score < C) return VALOR_ERR_ARG;
    if (((uintptr_t)featA & 15) || ((uintptr_t)storeB & 15) || ((uintptr_t)cand & 7) || ((uintptr_t)score & 3) || ((uintptr_t)maskA & 3) ||
        ((uintptr_t)wA & 3) || ((uintptr_t)wStoreB & 3))
        return VALOR_ERR_ARG;
    const int64_t blocks = (int64_t)NA * ((C + PAIR_BLOCK - 1) / PAIR_BLOCK);
    if (D > (1 << 20) || (int64_t)NA * T > 0x7fffffff || blocks > 0x7fffffff) return VALOR_ERR_ARG;
    const int tpb = T <= 16 ? 1 : (T <= 32 ? 2 : 4), vpb = Nv <= 16 ? 1 : (Nv <= 32 ? 2 : 4);
    const int TP = 16 * tpb;
    PairArgs p;
    p.fa = (const bf16_t*)featA; p.maskA = maskA; p.wA = wA; p.store = (const char*)storeB; p.wStore = wStoreB;
    p.cand = cand; p.ld_cand = ld_cand; p.score = score; p.ld_score = ld_score; p.NS = NS;
    p.NA = NA; p.C = C; p.T = T; p.Nv = Nv; p.D = D;
    p.seg = D < PAIR_LDS_BYTES / (TP * 2) ? D : PAIR_LDS_BYTES / (TP * 2);
    const unsigned lds = (unsigned)(TP * p.seg * 2);
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
#define PAIR_LAUNCH(TPB_, VPB_) hipLaunchKernelGGL((fine_score_pairs_kernel<TPB_, VPB_>), grid, dim3(256), lds, st, p)
    switch (tpb * 8 + vpb) {
        case 1 * 8 + 1: PAIR_LAUNCH(1, 1); break;
        case 1 * 8 + 2: PAIR_LAUNCH(1, 2); break;
        case 1 * 8 + 4: PAIR_LAUNCH(1, 4); break;
        case 2 * 8 + 1: PAIR_LAUNCH(2, 1); break;
        case 2 * 8 + 2: PAIR_LAUNCH(2, 2); break;
        case 2 * 8 + 4: PAIR_LAUNCH(2, 4); break;
        case 4 * 8 + 1: PAIR_LAUNCH(4, 1); break;
        case 4 * 8 + 2: PAIR_LAUNCH(4, 2); break;
        default: PAIR_LAUNCH(4, 4); break;
    }
#undef PAIR_LAUNCH
    return valor_launch_status();
}
