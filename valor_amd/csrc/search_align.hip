// Retrieval search, pair alignments: what valor_fine_score_pairs (search_pairs.hip) reduces away, kept. For every query and every clip
// of ITS OWN candidate list the kernel emits the maxima, the first arg maxima, the score split over the tokens of either side and,
// on request, the masked token similarities themselves.
//
// The law is that of fine_fused_fwd_kernel (contrastive_fused.hip) in its detail mode, for the pair (a, b = cand[a, c]):
//     x[t,v]   = S[t,v] * maskA[a,t]                                     (the clip mask is all ones and implicit)
//     a2b[t]   = max_v x, idx_a[t] = the first arg max;   b2a[v] = max_t x, idx_b[v] = the first arg max
//     score    = (sum_t wA[a,t] a2b[t] + sum_v wB[b,v] b2a[v]) / 2       the expression and the order of search_pairs.hip
// and the credits, every step fp32 and rounded on its own (no fma), so that a host loop reproduces them bit for bit:
//     termA[t] = 0.5 * (wA[t] * a2b[t]);    termB[v] = wB[v] != 0 ? 0.5 * (wB[v] * b2a[v]) : 0
//     credit_b[v] = termB[v], then + termA[t] for t ascending with idx_a[t] == v
//     credit_a[t] = termA[t], then + termB[v] for v ascending with idx_b[v] == t
// In exact arithmetic either credit array sums to the score. A candidate outside [0, NS) is never dereferenced: score -inf, index
// bytes 255, every other float 0.
//
// Shape: that of fine_score_pairs_kernel. A workgroup owns one query and PAIR_BLOCK consecutive candidates, the query's token rows
// sit in LDS as XOR images of mma.h, each of the four waves takes candidates in turn and reads the clip's fragments straight from the
// store through a buffer resource spanning exactly this clip, one step of look-ahead. The arg max is tracked as in the fused kernel:
// `>` in increasing slot order in-lane, then `min` over the lanes that hold the maximum. The credit scatter goes through ALIGN_WAVE_LDS
// bytes of LDS per wave beside the query image (terms and arg-max bytes by token, then lane = token walks the other side in ascending
// order); nothing crosses waves, so it needs no workgroup barrier. One launch, no workspace, no atomics.
#include "dpp.h"
#include "mma.h"

#define PAIR_BLOCK 16            // candidates per workgroup: four rounds of one candidate per wave
#define PAIR_OOB 0x7f000000      // a buffer offset past every clip: the range check returns zeros (padded token slots)
#define ALIGN_WAVE_LDS 640       // termA, termB fp32 [64]; idx_a, idx_b bytes [64]
#define ALIGN_LDS_BYTES (65536 - 4 * ALIGN_WAVE_LDS)      // the query image (a segment of it) beside the four waves' scatter space

struct AlignArgs {
    const bf16_t* fa;            // [NA, T, D]
    const float* maskA; const float* wA;
    const char* store;           // bf16 [NS, Nv, D]
    const float* wStore;         // [NS, Nv]
    const int64_t* cand; int64_t ld_cand;
    float* score;                // [NA, C]
    float* a2b; uint8_t* idx_a;  // [NA, C, T]
    float* b2a; uint8_t* idx_b;  // [NA, C, Nv]
    float* credit_a; float* credit_b;
    float* sim;                  // [NA, C, T, Nv]
    int64_t NS;
    int NA, C, T, Nv, D;
    int seg;                     // elements of D per LDS segment (a multiple of 64)
};

template <int TPB, int VPB>
__global__ __launch_bounds__(256) void fine_align_pairs_kernel(AlignArgs p) {
    typedef bf16_t T;
    constexpr int TP = 16 * TPB;
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    char* const smem = smem_all + 4 * ALIGN_WAVE_LDS;                 // the query image

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
    const bool credits = p.credit_a || p.credit_b;                    // workgroup-uniform

    float* const sTermA = (float*)(smem_all + wave * ALIGN_WAVE_LDS);
    float* const sTermB = sTermA + 64;
    uint8_t* const sIdxA = (uint8_t*)(sTermB + 64);
    uint8_t* const sIdxB = sIdxA + 64;

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
        const int64_t pair = (int64_t)a * p.C + c;
        const int64_t oT = pair * p.T, oV = pair * p.Nv;
        if (!live) {                                                  // no candidate: -inf, 255 and zeros
            if (p.score && lane == 0) p.score[pair] = NEG;
            if (lane < p.T) {
                if (p.a2b) { p.a2b[oT + lane] = 0.f; p.idx_a[oT + lane] = 255; }
                if (p.credit_a) p.credit_a[oT + lane] = 0.f;
            }
            if (lane < p.Nv) {
                if (p.b2a) { p.b2a[oV + lane] = 0.f; p.idx_b[oV + lane] = 255; }
                if (p.credit_b) p.credit_b[oV + lane] = 0.f;
            }
            if (p.sim) {
                const int n = p.T * p.Nv;
                for (int i = lane; i < n; i += 64) p.sim[oT * p.Nv + i] = 0.f;
            }
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

        if (p.sim) {                                                  // x itself: lane (fr, fg) holds x[t = mi*16 + fr][v = q*16 + 4*fg + r]
#pragma unroll
            for (int mi = 0; mi < TPB; ++mi) {
                const int t = mi * 16 + fr;
#pragma unroll
                for (int q = 0; q < VPB; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int v = q * 16 + 4 * fg + r;
                        if (t < p.T && v < p.Nv) p.sim[(oT + t) * p.Nv + v] = acc[q][mi][r];
                    }
            }
        }

        float ps = 0.f;           // per-lane partial of 2 * score
        // ---- A2B: max over the clip's tokens for every text token: in-lane over (q, r) in increasing v, then the four lane groups fg
#pragma unroll
        for (int mi = 0; mi < TPB; ++mi) {
            float best = NEG;
            int bv = 255;
#pragma unroll
            for (int q = 0; q < VPB; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float xv = acc[q][mi][r] + padV[q][r];
                    if (xv > best) { best = xv; bv = q * 16 + 4 * fg + r; }
                }
            float mx = fmaxf(best, __shfl_xor(best, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            int cnd = (best == mx) ? bv : 255;
            cnd = min(cnd, __shfl_xor(cnd, 16, 64));
            cnd = min(cnd, __shfl_xor(cnd, 32, 64));
            if (fg == 0) ps += mx * wAl[mi];                          // counted once per t
            const int t = mi * 16 + fr;
            if (fg == 0 && t < p.T) {
                if (p.a2b) { p.a2b[oT + t] = mx; p.idx_a[oT + t] = (uint8_t)cnd; }
                if (credits) { sTermA[t] = __fmul_rn(0.5f, __fmul_rn(wAl[mi], mx)); sIdxA[t] = (uint8_t)cnd; }
            }
        }
        // ---- B2A: max over the text's tokens for every clip token: in-lane over the row blocks (increasing t), then the DPP row
#pragma unroll
        for (int q = 0; q < VPB; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float best = NEG;
                int bt = 255;
#pragma unroll
                for (int mi = 0; mi < TPB; ++mi) {
                    const float xv = acc[q][mi][r] + padT[mi];
                    if (xv > best) { best = xv; bt = mi * 16 + fr; }
                }
                const float mx = row16_max(best);
                const int cnd = row16_min((best == mx) ? bt : 255);
                if (fr == 0) ps += (wBl[q][r] != 0.f) ? mx * wBl[q][r] : 0.f;      // padded slots: weight 0 (and mx may be -inf)
                const int v = q * 16 + 4 * fg + r;
                if (fr == 0 && v < p.Nv) {
                    if (p.b2a) { p.b2a[oV + v] = mx; p.idx_b[oV + v] = (uint8_t)cnd; }
                    if (credits) {
                        sTermB[v] = (wBl[q][r] != 0.f) ? __fmul_rn(0.5f, __fmul_rn(wBl[q][r], mx)) : 0.f;
                        sIdxB[v] = (uint8_t)cnd;
                    }
                }
            }
        float s = row16_sum(ps);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (p.score && lane == 0) p.score[pair] = 0.5f * s;

        // ---- credits: lane = token; the other side's terms are added in ascending token order, one rounded addition each
        if (credits) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (p.credit_b && lane < p.Nv) {
                float cr = sTermB[lane];
                for (int t = 0; t < p.T; ++t)
                    if (sIdxA[t] == lane) cr = __fadd_rn(cr, sTermA[t]);
                p.credit_b[oV + lane] = cr;
            }
            if (p.credit_a && lane < p.T) {
                float cr = sTermA[lane];
                for (int v = 0; v < p.Nv; ++v)
                    if (sIdxB[v] == lane) cr = __fadd_rn(cr, sTermB[v]);
                p.credit_a[oT + lane] = cr;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    // the next round's terms are written after these reads
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// featA bf16 [NA, T, D]; storeB bf16 [NS, Nv, D] with wStoreB fp32 [NS, Nv]; cand int64 [NA, ld_cand]; the outputs dense, C columns per query
extern "C" int valor_fine_align_pairs(void* stream, const void* featA, const float* maskA, const float* wA, const void* storeB,
                                      const float* wStoreB, int64_t NS, const int64_t* cand, int64_t ld_cand, int NA, int C, int T, int Nv,
                                      int D, float* score, float* a2b, uint8_t* idx_a, float* b2a, uint8_t* idx_b, float* credit_a,
                                      float* credit_b, float* sim) {
    if (NA == 0 || C == 0) return VALOR_OK;
    if (NA < 0 || C < 0 || NS < 0 || T <= 0 || T > 64 || Nv <= 0 || Nv > 64 || D <= 0 || (D % 64) != 0) return VALOR_ERR_ARG;
    if (!featA || !maskA || !wA || !storeB || !wStoreB || !cand || ld_cand < C) return VALOR_ERR_ARG;
    if ((a2b != nullptr) != (idx_a != nullptr) || (b2a != nullptr) != (idx_b != nullptr)) return VALOR_ERR_ARG;
    if (((uintptr_t)featA & 15) || ((uintptr_t)storeB & 15) || ((uintptr_t)cand & 7) || ((uintptr_t)maskA & 3) || ((uintptr_t)wA & 3) ||
        ((uintptr_t)wStoreB & 3) || ((uintptr_t)score & 3) || ((uintptr_t)a2b & 3) || ((uintptr_t)b2a & 3) || ((uintptr_t)credit_a & 3) ||
        ((uintptr_t)credit_b & 3) || ((uintptr_t)sim & 3))
        return VALOR_ERR_ARG;
    const int64_t blocks = (int64_t)NA * ((C + PAIR_BLOCK - 1) / PAIR_BLOCK);
    if (D > (1 << 20) || (int64_t)NA * T > 0x7fffffff || blocks > 0x7fffffff) return VALOR_ERR_ARG;
    if (!score && !a2b && !b2a && !credit_a && !credit_b && !sim) return VALOR_OK;      // nothing asked for
    const int tpb = T <= 16 ? 1 : (T <= 32 ? 2 : 4), vpb = Nv <= 16 ? 1 : (Nv <= 32 ? 2 : 4);
    const int TP = 16 * tpb;
    AlignArgs p;
    p.fa = (const bf16_t*)featA; p.maskA = maskA; p.wA = wA; p.store = (const char*)storeB; p.wStore = wStoreB;
    p.cand = cand; p.ld_cand = ld_cand; p.score = score; p.a2b = a2b; p.idx_a = idx_a; p.b2a = b2a; p.idx_b = idx_b;
    p.credit_a = credit_a; p.credit_b = credit_b; p.sim = sim; p.NS = NS;
    p.NA = NA; p.C = C; p.T = T; p.Nv = Nv; p.D = D;
    const int seg_max = ALIGN_LDS_BYTES / (TP * 2) / 64 * 64;
    p.seg = D < seg_max ? D : seg_max;
    const unsigned lds = (unsigned)(4 * ALIGN_WAVE_LDS + TP * p.seg * 2);
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
#define ALIGN_LAUNCH(TPB_, VPB_) hipLaunchKernelGGL((fine_align_pairs_kernel<TPB_, VPB_>), grid, dim3(256), lds, st, p)
    switch (tpb * 8 + vpb) {
        case 1 * 8 + 1: ALIGN_LAUNCH(1, 1); break;
        case 1 * 8 + 2: ALIGN_LAUNCH(1, 2); break;
        case 1 * 8 + 4: ALIGN_LAUNCH(1, 4); break;
        case 2 * 8 + 1: ALIGN_LAUNCH(2, 1); break;
        case 2 * 8 + 2: ALIGN_LAUNCH(2, 2); break;
        case 2 * 8 + 4: ALIGN_LAUNCH(2, 4); break;
        case 4 * 8 + 1: ALIGN_LAUNCH(4, 1); break;
        case 4 * 8 + 2: ALIGN_LAUNCH(4, 2); break;
        default: ALIGN_LAUNCH(4, 4); break;
    }
#undef ALIGN_LAUNCH
    return valor_launch_status();
}
