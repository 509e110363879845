// The n-gram scoring core of the caption kernels: CIDEr(-D) and the BLEU integers of one hypothesis row against the reference captions of
// its clip. reward.hip (the SCST reward) and capeval.hip (the evaluation metrics) are this core plus what is their own; the table types
// valor_reward_tables / valor_capeval_tables (include/valor_hip.h) carry the fields read here under the same names, hence `class Tables`.
//
// Keys: an n-gram (t_0 .. t_{n-1}) is ONE 64-bit integer, (t_i + 1) in 16-bit field i, unused fields 0: exact, no hashing, n is the number
// of non-zero fields. A hypothesis token outside [0, vocab) takes the code 65535, which no table key carries: it matches nothing, and two
// such n-grams count as the same n-gram only if their raw tokens agree (what a dictionary of token tuples does).
//
// Tiling: ONE workgroup of four waves per hypothesis row. What lives where (NgramLds, 35 KB):
//   tok  [128] int64   the row's raw tokens          key [512] uint64  slot n * 128 + i = the (n + 1)-gram starting at token i
//   tf   [512] int32   the n-gram's count on its FIRST occurrence, 0 on repeats and on empty slots
//   x    [512] fp64    tf * idf of the slot (0 where tf == 0)
//   rkey / rval [1536] the clip's reference keys and tf-idf values (CSR, sorted per reference), staged when they fit; a clip with
//                      more entries is probed in global memory through the same (flat) pointers.
// Passes (a barrier between them; a function that holds one is called by all 256 threads, and says so):
//   ng_load_row     1. load the tokens, find the first eos (ballot per wave, minimum over the four waves), form the keys;
//                   2. count duplicates: slot (n, i) compares with the other starts of its n (at most 128 compares of one 64-bit key);
//   ng_score_slots  3. idf of every first occurrence by binary search in the global table (absent: ref_len), x = tf * idf, the squares
//                      for the four hypothesis norms (ng_norms, after the caller's barrier); in the same pass the BLEU clipped counts
//                      (binary search in the clip's merged maximum-count list) and the closest reference length;
//   ng_cider        4. wave w takes the references w, w + 4, ..; a lane takes the slots lane, lane + 64, .. (two per n), probes the
//                      reference's sorted list, and the four clipped dot products are reduced over the wave by shuffles;
//   ng_cider_total, ng_correct, ng_bleu: what one thread combines after the last barrier.
// Arithmetic: every sum, the norms and exp / sqrt / pow are fp64 (BLEU's 1e-15 terms do not survive fp32). Every reduction has a fixed
// order (shuffle trees, then LDS slots summed by one thread; the only atomics are integer ones in LDS): two launches on the same input
// return the same bits. The idf values and the reference tf-idf values are the host's bits: the kernels never evaluate log.
#pragma once
#include "common.h"
#include "../../include/valor_hip.h"
#include <math.h>

#define NG_THREADS 256
#define NG_WAVES 4
#define NG_MAXL 128
#define NG_SLOTS (4 * NG_MAXL)
#define NG_STAGE 1536
#define NG_UNKNOWN 65535ull

struct NgramLds {
    int64_t tok[NG_MAXL];
    uint64_t key[NG_SLOTS];
    double x[NG_SLOTS];
    uint64_t rkey[NG_STAGE];
    double rval[NG_STAGE];
    double sq[NG_WAVES][2], norm[4], score[NG_WAVES][4];
    unsigned long long closest;
    int tf[NG_SLOTS];
    int cut[NG_WAVES], correct[NG_WAVES][2];
};

// index of `k` in the sorted keys[lo, hi), -1 if absent
DEVINL int ng_find(const uint64_t* keys, int lo, int hi, uint64_t k) {
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && keys[lo] == k) ? lo : -1;
}
DEVINL double ng_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
DEVINL int ng_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (prod_{j <= k} (correct_j + 1e-15) / (guess_j + 1e-9))^(1 / k), k = 1..4, with the brevity penalty (bleu_scorer.py:234-242, 251-259)
template <typename I>
DEVINL void ng_bleu(const I* correct, const I* guess, I testlen, I reflen, double* out) {
    double b = 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b *= ((double)correct[k] + 1e-15) / ((double)guess[k] + 1e-9);
        out[k] = pow(b, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)testlen + 1e-15) / ((double)reflen + 1e-9);
    if (ratio < 1.0) {
        const double bp = exp(1.0 - 1.0 / ratio);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] *= bp;
    }
}

// the references [ref0, ref1) of the row's clip; empty for a clip index outside the table (block-uniform: the caller returns on it)
template <class Tables>
DEVINL void ng_clip_refs(const Tables& T, int c, int& ref0, int& ref1) {
    ref0 = ref1 = 0;
    if (c >= 0 && c < T.n_clips) { ref0 = T.clip_ref_ptr[c]; ref1 = T.clip_ref_ptr[c + 1]; }
}

// Passes 1 and 2 (ALL threads: two barriers inside, none at the end) -> the row's length. k0 = the clip's first reference key, staged =
// its lists are in S.rkey / S.rval.
template <class Tables>
DEVINL int ng_load_row(NgramLds& S, const Tables& T, const int64_t* __restrict__ seq, int64_t ld, int L, int64_t eos, int vocab, int ref0,
                       int ref1, int& k0, bool& staged) {
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t t = eos;
    if (tid < L) t = seq[(int64_t)r * ld + tid];
    if (tid < NG_MAXL) S.tok[tid] = t;
    {
        const unsigned long long hit = __ballot(tid < L && t == eos);
        if (lane == 0) S.cut[wave] = hit ? wave * 64 + __builtin_ctzll(hit) : L;
        if (tid == 0) S.closest = ~0ull;
    }
    // the clip's reference lists into LDS while the tokens settle
    k0 = T.ref_key_ptr[ref0];
    const int k1 = T.ref_key_ptr[ref1];
    staged = k1 - k0 <= NG_STAGE;
    if (staged)
        for (int i = tid; i < k1 - k0; i += NG_THREADS) { S.rkey[i] = T.ref_keys[k0 + i]; S.rval[i] = T.ref_vals[k0 + i]; }
    __syncthreads();
    int len = S.cut[0];
#pragma unroll
    for (int w = 1; w < NG_WAVES; ++w) len = S.cut[w] < len ? S.cut[w] : len;
    len = len < L ? len : L;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * NG_THREADS, n = s >> 7, i = s & (NG_MAXL - 1);          // the (n + 1)-gram starting at i
        uint64_t key = 0;
        if (i + n < len) {
            for (int j = 0; j <= n; ++j) {
                const int64_t w = S.tok[i + j];
                const uint64_t code = (w >= 0 && w < (int64_t)vocab) ? (uint64_t)w + 1 : NG_UNKNOWN;
                key |= code << (16 * j);
            }
        }
        S.key[s] = key;
    }
    __syncthreads();
    // counts: tf on the first occurrence of an n-gram, 0 on its repeats
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * NG_THREADS, n = s >> 7, i = s & (NG_MAXL - 1);
        const uint64_t key = S.key[s];
        int cnt = 0;
        bool first = true;
        if (key) {
            const bool unk = ((key & 0xffff) == NG_UNKNOWN) || (((key >> 16) & 0xffff) == NG_UNKNOWN) || (((key >> 32) & 0xffff) == NG_UNKNOWN) ||
                             ((key >> 48) == NG_UNKNOWN);
            const int starts = len - n;
            for (int j = 0; j < starts; ++j) {
                bool eq = S.key[(n << 7) + j] == key;
                if (eq && unk)
                    for (int q = 0; q <= n; ++q) eq = eq && S.tok[i + q] == S.tok[j + q];
                cnt += eq ? 1 : 0;
                first = first && !(eq && j < i);
            }
        }
        S.tf[s] = (key && first) ? cnt : 0;
    }
    return len;
}

// Pass 3 (after the caller's barrier behind ng_load_row; the caller closes it with a barrier of its own): S.x, the wave sums of the
// squares and of the BLEU clipped counts, S.closest = (distance, length) of the closest reference length.
template <class Tables>
DEVINL void ng_score_slots(NgramLds& S, const Tables& T, int c, int ref0, int ref1, int len) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = T.clip_bleu_ptr[c], b1 = T.clip_bleu_ptr[c + 1];
    double sq[2];
    int corr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * NG_THREADS;
        const int tf = S.tf[s];
        double x = 0.0;
        int cc = 0;
        if (tf) {
            const uint64_t key = S.key[s];
            const int g = T.n_global > 0 ? ng_find(T.g_keys, 0, T.n_global, key) : -1;
            x = (double)tf * (g >= 0 ? T.g_idf[g] : T.ref_len);
            const int m = ng_find(T.bleu_keys, b0, b1, key);
            if (m >= 0) { const int mc = T.bleu_cnt[m]; cc = mc < tf ? mc : tf; }
        }
        S.x[s] = x;
        sq[h] = ng_wave_sum(x * x);
        corr[h] = ng_wave_sum(cc);
    }
    if (lane == 0) { S.sq[wave][0] = sq[0]; S.sq[wave][1] = sq[1]; S.correct[wave][0] = corr[0]; S.correct[wave][1] = corr[1]; }
    for (int q = ref0 + tid; q < ref1; q += NG_THREADS) {
        const int l = T.ref_tokens[q];
        const unsigned d = (unsigned)(l > len ? l - len : len - l);
        atomicMin(&S.closest, ((unsigned long long)d << 32) | (unsigned)l);          // integer: (distance, length), ties to the shorter
    }
}

// the four hypothesis norms (after the barrier that closes pass 3; a barrier before ng_cider reads them). Slots 0..127 (n = 1) belong to
// waves 0, 1 at h = 0; 128..255 (n = 2) to waves 2, 3 at h = 0; n = 3, 4 the same at h = 1
DEVINL void ng_norms(NgramLds& S) {
    const int tid = threadIdx.x;
    if (tid < 4) S.norm[tid] = sqrt(S.sq[(tid & 1) * 2][tid >> 1] + S.sq[(tid & 1) * 2 + 1][tid >> 1]);
}

// Pass 4: CIDEr-D against every reference of the clip -> S.score[wave][n] (a barrier before ng_cider_total reads them)
template <class Tables>
DEVINL void ng_cider(NgramLds& S, const Tables& T, int ref0, int ref1, int k0, bool staged, int len) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t* rkeys = staged ? S.rkey : T.ref_keys + k0;
    const double* rvals = staged ? S.rval : T.ref_vals + k0;
    const int lh = len > 1 ? len - 1 : 0;                  // the hypothesis' bigram count: the reference's "length"
    double score[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = ref0 + wave; q < ref1; q += NG_WAVES) {
        const int lo = T.ref_key_ptr[q] - k0, hi = T.ref_key_ptr[q + 1] - k0;
        double val[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = lane + 64 * k;
            if (S.tf[s]) {
                const int m = ng_find(rkeys, lo, hi, S.key[s]);
                if (m >= 0) {
                    const double x = S.x[s], y = rvals[m];
                    val[k >> 1] += (x < y ? x : y) * y;
                }
            }
        }
        const double delta = (double)(lh - T.ref_bigrams[q]);
        const double pen = exp(-(delta * delta) / (2.0 * 6.0 * 6.0));
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double v = ng_wave_sum(val[n]);
            const double nh = S.norm[n], nr = T.ref_norm[(int64_t)q * 4 + n];
            if (nh != 0.0 && nr != 0.0) v /= nh * nr;
            score[n] += v * pen;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) S.score[wave][n] = score[n];
    }
}

// what one thread combines: the mean over n and references, times 10
DEVINL double ng_cider_total(const NgramLds& S, int ref0, int ref1) {
    double sum = 0.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) sum += (S.score[0][n] + S.score[1][n]) + (S.score[2][n] + S.score[3][n]);
    return sum / 4.0 / (double)(ref1 - ref0) * 10.0;
}
// ... and BLEU's integers of a row of `len` tokens: the clipped counts, the guesses max(0, len - k), the closest reference length
DEVINL int ng_correct(const NgramLds& S, int len, int* correct, int* guess) {
    correct[0] = S.correct[0][0] + S.correct[1][0];
    correct[1] = S.correct[2][0] + S.correct[3][0];
    correct[2] = S.correct[0][1] + S.correct[1][1];
    correct[3] = S.correct[2][1] + S.correct[3][1];
#pragma unroll
    for (int k = 0; k < 4; ++k) guess[k] = len - k > 0 ? len - k : 0;
    return (int)(unsigned)(S.closest & 0xffffffffull);
}

// The geometry and table pointers both entry points take (host): VALOR_ERR_ARG or VALOR_OK. No rows need no pointers.
template <class Tables>
static int ng_check_args(const void* seq, int64_t ld, int R, int L, int64_t eos, int vocab, const void* clip_idx, const Tables* t) {
    if (R < 0 || L < 1 || L > NG_MAXL || vocab < 1 || vocab > 65534 || eos < 0 || eos >= vocab || ld < L) return VALOR_ERR_ARG;
    if (R == 0) return VALOR_OK;
    if (!seq || !clip_idx || !t) return VALOR_ERR_ARG;
    if (!t->clip_ref_ptr || !t->ref_key_ptr || !t->ref_keys || !t->ref_vals || !t->ref_norm || !t->ref_bigrams || !t->ref_tokens ||
        !t->clip_bleu_ptr || !t->bleu_keys || !t->bleu_cnt)
        return VALOR_ERR_ARG;
    if (t->n_clips < 1 || t->n_global < 0 || (t->n_global > 0 && (!t->g_keys || !t->g_idf))) return VALOR_ERR_ARG;
    return VALOR_OK;
}
