// What the two row selections share (search.hip: valor_topk_rows; search_select.hip: valor_topk_rows_select): the orderable key of a
// value, the total order, the 1024-column load step and the host's segment plan. See search.hip for the order and the plan.
#pragma once
#include "common.h"
#include <math.h>

#define TK_THREADS 256
#define TK_CAP 512
#define TK_STEP 1024
#define TK_NONE INT64_MAX

DEVINL uint32_t tk_ord(float v) {
    if (v != v) return 0u;
    if (v == 0.f) return 0x80000000u;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
DEVINL float tk_val(uint32_t o) {
    if (o == 0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
DEVINL bool tk_beats(uint32_t oa, int64_t ia, uint32_t ob, int64_t ib) { return oa > ob || (oa == ob && ia < ib); }

template <bool VEC4> DEVINL void tk_load4(const float* row, int64_t j0, int C, float* v) {
    const float nanv = __uint_as_float(0x7fc00000u);
    if constexpr (VEC4) {
        const int64_t j = j0 + 4 * (int)threadIdx.x;
        if (j < C) {                    // ld % 4 == 0 and j % 4 == 0: j + 3 < ld, the load stays inside the row
            const f32x4_t t = *(const f32x4_t*)(row + j);
            v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
        } else {
            v[0] = v[1] = v[2] = v[3] = nanv;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t j = j0 + (int)threadIdx.x + TK_THREADS * e;
            v[e] = (j < C) ? row[j] : nanv;
        }
    }
}
template <bool VEC4> DEVINL int64_t tk_col(int64_t j0, int e) { return VEC4 ? j0 + 4 * (int)threadIdx.x + e : j0 + (int)threadIdx.x + TK_THREADS * e; }

// ---------------------------------------------------------------- the accumulator (search.hip describes it; GROUPED: search_select.hip)
// TK_CAP keys in LDS, a counter, and the running threshold in registers. GROUPED adds a third column, the candidate's group id, and a
// compaction that keeps one entry per group id >= 0.
template <bool GROUPED> struct TkState {
    uint32_t* ord;      // LDS [TK_CAP]
    int64_t* idx;       // LDS [TK_CAP]
    int* grp;           // LDS [TK_CAP], 16-byte aligned (GROUPED only)
    int* cnt;           // LDS
    int* wsum;          // LDS [TK_THREADS / 64]: survivors per wave of a compaction (GROUPED only)
    uint32_t thr_o;     // the k-th best (GROUPED: the k-th best distinct representative) so far, uniform over the workgroup;
    int64_t thr_i;      // (0, TK_NONE) = none
    int k;
};

// best first; every thread of the workgroup; ends behind a barrier
template <bool GROUPED> DEVINL void tk_sort(const TkState<GROUPED>& s) {
    const int tid = threadIdx.x;
    for (int size = 2; size <= TK_CAP; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            const int lo = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), hi = lo | j;
            const uint32_t oa = s.ord[lo], ob = s.ord[hi];
            const int64_t ia = s.idx[lo], ib = s.idx[hi];
            const bool fwd = (lo & size) == 0;
            if (fwd ? tk_beats(ob, ib, oa, ia) : tk_beats(oa, ia, ob, ib)) {
                s.ord[lo] = ob; s.idx[lo] = ib;
                s.ord[hi] = oa; s.idx[hi] = ia;
                if constexpr (GROUPED) {
                    const int ga = s.grp[lo];
                    s.grp[lo] = s.grp[hi];
                    s.grp[hi] = ga;
                }
            }
            __syncthreads();
        }
    }
}

// All TK_CAP slots hold a key (the sentinel included). Sort, keep the k best and make the k-th the threshold; returns the number kept.
// GROUPED: every entry whose group id (>= 0) appeared EARLIER in sorted order is dropped first and the survivors move to the front in
// order: slots 0 .. min(n, k) - 1 then hold the best distinct representatives, n being their number, slots n .. k - 1 the sentinel,
// and the threshold is the k-th representative, or none when n < k. Duplicates are found by an all-pairs scan: thread t owns the
// entries 2 t and 2 t + 1 and compares their ids with every earlier entry's, read as 16-byte LDS broadcasts (at most 128 reads a
// thread); a ballot prefix sum places the survivors. Every thread of the workgroup; ends behind a barrier.
template <bool GROUPED> DEVINL int tk_compact(TkState<GROUPED>& s) {
    tk_sort(s);
    int n = TK_CAP;
    if constexpr (GROUPED) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int p0 = 2 * tid, p1 = p0 + 1;
        const int g0 = s.grp[p0], g1 = s.grp[p1];
        bool dup0 = false, dup1 = g1 == g0;
        // this wave owns the entries [128 wave, 128 wave + 128): everything before them is earlier, nothing behind them matters to it.
        // Bitwise, not short-circuit: no branches in the scan.
        const int qown = 128 * wave;
        for (int q = 0; q < qown; q += 4) {
            const int4 gq = *(const int4*)(s.grp + q);
            dup0 |= (gq.x == g0) | (gq.y == g0) | (gq.z == g0) | (gq.w == g0);
            dup1 |= (gq.x == g1) | (gq.y == g1) | (gq.z == g1) | (gq.w == g1);
        }
        for (int q = qown; q < qown + 128; q += 4) {
            const int4 gq = *(const int4*)(s.grp + q);
            const bool e0 = q + 0 < p0, e1 = q + 1 < p0, e2 = q + 2 < p0, e3 = q + 3 < p0;
            dup0 |= (e0 & (gq.x == g0)) | (e1 & (gq.y == g0)) | (e2 & (gq.z == g0)) | (e3 & (gq.w == g0));
            dup1 |= (e0 & (gq.x == g1)) | (e1 & (gq.y == g1)) | (e2 & (gq.z == g1)) | (e3 & (gq.w == g1));
        }
        const bool f0 = !(dup0 && g0 >= 0), f1 = !(dup1 && g1 >= 0);  // an id < 0 is a group of its own
        const uint32_t o0 = s.ord[p0], o1 = s.ord[p1];
        const int64_t i0 = s.idx[p0], i1 = s.idx[p1];
        const uint64_t b0 = __ballot(f0), b1 = __ballot(f1), below = (1ull << lane) - 1ull;
        if (lane == 0) s.wsum[wave] = __popcll(b0) + __popcll(b1);
        __syncthreads();                // every entry is in registers: the survivors may move
        int base = 0;
        n = 0;
        for (int w = 0; w < TK_THREADS / 64; ++w) {
            const int c = s.wsum[w];
            base += w < wave ? c : 0;
            n += c;
        }
        const int d0 = base + __popcll(b0 & below) + __popcll(b1 & below), d1 = d0 + (f0 ? 1 : 0);
        if (f0 && d0 < s.k) { s.ord[d0] = o0; s.idx[d0] = i0; s.grp[d0] = g0; }
        if (f1 && d1 < s.k) { s.ord[d1] = o1; s.idx[d1] = i1; s.grp[d1] = g1; }
        for (int p = n + tid; p < s.k; p += TK_THREADS) { s.ord[p] = 0u; s.idx[p] = TK_NONE; s.grp[p] = -1; }
        __syncthreads();
    }
    if (n >= s.k) {
        s.thr_o = s.ord[s.k - 1];
        s.thr_i = s.idx[s.k - 1];
        n = s.k;
    } else {
        s.thr_o = 0u;
        s.thr_i = TK_NONE;
    }
    return n;
}

template <bool GROUPED>
DEVINL void tk_init(TkState<GROUPED>& s, uint32_t* ord, int64_t* idx, int* cnt, int k, int* grp = nullptr, int* wsum = nullptr) {
    s.ord = ord; s.idx = idx; s.grp = grp; s.cnt = cnt; s.wsum = wsum; s.k = k;
    s.thr_o = 0u; s.thr_i = TK_NONE;
    if (threadIdx.x == 0) *cnt = 0;
    __syncthreads();
}

// Every thread of the workgroup calls this together, each with its own key (GROUPED: and group id) or want = false.
template <bool GROUPED> DEVINL void tk_push(TkState<GROUPED>& s, bool want, uint32_t o, int64_t i, int g = -1) {
    const int lane = threadIdx.x & 63;
    while (__syncthreads_or(want)) {
        const uint64_t m = __ballot(want);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(s.cnt, __popcll(m));
            base = __shfl(base, leader, 64);
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            if (want && pos < TK_CAP) {
                s.ord[pos] = o; s.idx[pos] = i;
                if constexpr (GROUPED) s.grp[pos] = g;
                want = false;
            }
        }
        __syncthreads();
        if (*s.cnt >= TK_CAP) {           // full (slots 0 .. TK_CAP - 1 are all written): keep the k best, raise the threshold
            const int n = tk_compact(s);  // ends behind a barrier: every thread has read the counter
            if (threadIdx.x == 0) *s.cnt = n;
            want = want && tk_beats(o, i, s.thr_o, s.thr_i);
        }
    }
}

// pad with the sentinel and compact: the k best are slots 0 .. k - 1 afterwards, the sentinel behind them
template <bool GROUPED> DEVINL void tk_finish(TkState<GROUPED>& s) {
    const int n = *s.cnt;               // <= TK_CAP: tk_push leaves no full buffer behind
    for (int p = threadIdx.x; p < TK_CAP; p += TK_THREADS)
        if (p >= n) {
            s.ord[p] = 0u; s.idx[p] = TK_NONE;
            if constexpr (GROUPED) s.grp[p] = -1;
        }
    __syncthreads();
    if constexpr (GROUPED) tk_compact(s);
    else tk_sort(s);
}

// ---------------------------------------------------------------- host
static inline int64_t tk_align16(int64_t n) { return (n + 15) / 16 * 16; }
// segments of a row: at most one per 4096 columns (C = 4099: two segments of 3072), each a multiple of TK_STEP columns, and no more than fill
// the machine a few times over (about 2048 workgroups in all)
static inline void tk_plan(int R, int C, int* nseg, int* seg) {
    const int64_t most = ((int64_t)C + 4095) / 4096, want = (2048 + (int64_t)R - 1) / R;
    int64_t n = most < want ? most : want;
    if (n < 1) n = 1;
    int64_t sz = (((int64_t)C + n - 1) / n + TK_STEP - 1) / TK_STEP * TK_STEP;
    if (sz < TK_STEP) sz = TK_STEP;
    n = ((int64_t)C + sz - 1) / sz;
    *nseg = (int)(n < 1 ? 1 : n);
    *seg = (int)sz;
}
// workspace layout: [indices: R * nseg * k int64 | keys: R * nseg * k uint32], each part 16-byte aligned
static inline int64_t tk_workspace(int R, int C, int k) {
    int nseg, seg;
    tk_plan(R, C, &nseg, &seg);
    const int64_t n = (int64_t)R * nseg * k;
    return tk_align16(n * 8) + tk_align16(n * 4);
}
