// The caption reward of self-critical sequence training on the device: CIDEr-D + BLEU-4 of every hypothesis row against the reference
// captions of its clip (valor_amd/scst.py states the rules; scorer/cider_scorer.py:119-200, scorer/bleu_scorer.py:202-250 'closest').
// See include/valor_hip.h for the contract and the table format (valor_reward_tables, built by scst.reward_tables).
//
// Keys: an n-gram (t_0 .. t_{n-1}) is ONE 64-bit integer, (t_i + 1) in 16-bit field i, unused fields 0: exact, no hashing, n is the number
// of non-zero fields. A hypothesis token outside [0, vocab) takes the code 65535, which no table key carries: it matches nothing, and two
// such n-grams count as the same n-gram only if their raw tokens agree (what a dictionary of token tuples does).
//
// Tiling: ONE workgroup of four waves per hypothesis row; a launch of R workgroups scores sample and greedy rows of every group at once.
// What lives where (LDS, 35 KB: four workgroups per CU):
//   tok  [128] int64   the row's raw tokens          key [512] uint64  slot n * 128 + i = the (n + 1)-gram starting at token i
//   tf   [512] int32   the n-gram's count on its FIRST occurrence, 0 on repeats and on empty slots
//   x    [512] fp64    tf * idf of the slot (0 where tf == 0)
//   rkey / rval [1536] the clip's reference keys and tf-idf values (CSR, sorted per reference), staged when they fit; a clip with
//                      more entries is probed in global memory through the same (flat) pointers.
// Passes (barriers between them):
//   1. load the tokens, find the first eos (ballot per wave, minimum over the four waves), form the keys;
//   2. count duplicates: slot (n, i) compares with the other starts of its n (at most 128 compares of one 64-bit key);
//   3. idf of every first occurrence by binary search in the global table (absent: ref_len), x = tf * idf; the four hypothesis norms;
//      in the same pass the BLEU clipped counts (binary search in the clip's merged maximum-count list) and the closest reference length;
//   4. CIDEr-D: wave w takes the references w, w + 4, ..; a lane takes the slots lane, lane + 64, .. (two per n), probes the reference's
//      sorted list, and the four clipped dot products are reduced over the wave by shuffles;
//   5. thread 0 combines: mean over n and references, times 10; BLEU-4 with its brevity penalty; reward = the sum.
// Arithmetic: every sum, the norms and exp / sqrt / pow are fp64 (BLEU's 1e-15 terms do not survive fp32). Every reduction has a fixed
// order (shuffle trees, then LDS slots summed by one thread; the only atomics are integer min / add in LDS): two launches on the same
// input return the same bits. The idf values and the reference tf-idf values are the host's bits: the kernel never evaluates log.
#include "common.h"
#include "../../include/valor_hip.h"
#include <math.h>

#define RW_THREADS 256
#define RW_WAVES 4
#define RW_MAXL 128
#define RW_SLOTS (4 * RW_MAXL)
#define RW_STAGE 1536
#define RW_UNKNOWN 65535ull

typedef valor_reward_tables RewardTables;          // the one definition: include/valor_hip.h

// index of `k` in the sorted keys[lo, hi), -1 if absent
DEVINL int rw_find(const uint64_t* keys, int lo, int hi, uint64_t k) {
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && keys[lo] == k) ? lo : -1;
}
DEVINL double rw_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
DEVINL int rw_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(RW_THREADS) void caption_reward_kernel(const int64_t* __restrict__ seq, int64_t ld, int L, int64_t eos, int vocab,
                                                                    const int32_t* __restrict__ clip_idx, RewardTables T,
                                                                    double* __restrict__ reward, double* __restrict__ cider,
                                                                    double* __restrict__ bleu) {
    __shared__ int64_t sh_tok[RW_MAXL];
    __shared__ uint64_t sh_key[RW_SLOTS];
    __shared__ double sh_x[RW_SLOTS];
    __shared__ int sh_tf[RW_SLOTS];
    __shared__ uint64_t sh_rkey[RW_STAGE];
    __shared__ double sh_rval[RW_STAGE];
    __shared__ double sh_sq[RW_WAVES][2], sh_norm[4], sh_score[RW_WAVES][4];
    __shared__ int sh_cut[RW_WAVES], sh_correct[RW_WAVES][2];
    __shared__ unsigned long long sh_closest;

    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const int c = clip_idx[r];
    int ref0 = 0, ref1 = 0;
    if (c >= 0 && c < T.n_clips) { ref0 = T.clip_ref_ptr[c]; ref1 = T.clip_ref_ptr[c + 1]; }
    if (ref1 <= ref0) {                                    // no such clip, or a clip without references: no score (block-uniform)
        if (tid == 0) {
            reward[r] = nanv;
            if (cider) cider[r] = nanv;
            if (bleu) bleu[r] = nanv;
        }
        return;
    }

    // ---- pass 1: tokens, the cut, the keys
    int64_t t = eos;
    if (tid < L) t = seq[(int64_t)r * ld + tid];
    if (tid < RW_MAXL) sh_tok[tid] = t;
    {
        const unsigned long long hit = __ballot(tid < L && t == eos);
        if (lane == 0) sh_cut[wave] = hit ? wave * 64 + __builtin_ctzll(hit) : L;
        if (tid == 0) sh_closest = ~0ull;
    }
    // the clip's reference lists into LDS while the tokens settle
    const int k0 = T.ref_key_ptr[ref0], k1 = T.ref_key_ptr[ref1];
    const bool staged = k1 - k0 <= RW_STAGE;
    if (staged)
        for (int i = tid; i < k1 - k0; i += RW_THREADS) { sh_rkey[i] = T.ref_keys[k0 + i]; sh_rval[i] = T.ref_vals[k0 + i]; }
    __syncthreads();
    int len = sh_cut[0];
#pragma unroll
    for (int w = 1; w < RW_WAVES; ++w) len = sh_cut[w] < len ? sh_cut[w] : len;
    len = len < L ? len : L;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * RW_THREADS, n = s >> 7, i = s & (RW_MAXL - 1);          // the (n + 1)-gram starting at i
        uint64_t key = 0;
        if (i + n < len) {
            for (int j = 0; j <= n; ++j) {
                const int64_t w = sh_tok[i + j];
                const uint64_t code = (w >= 0 && w < (int64_t)vocab) ? (uint64_t)w + 1 : RW_UNKNOWN;
                key |= code << (16 * j);
            }
        }
        sh_key[s] = key;
    }
    __syncthreads();

    // ---- pass 2: counts. tf on the first occurrence of an n-gram, 0 on its repeats
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * RW_THREADS, n = s >> 7, i = s & (RW_MAXL - 1);
        const uint64_t key = sh_key[s];
        int cnt = 0;
        bool first = true;
        if (key) {
            const bool unk = ((key & 0xffff) == RW_UNKNOWN) || (((key >> 16) & 0xffff) == RW_UNKNOWN) || (((key >> 32) & 0xffff) == RW_UNKNOWN) ||
                             ((key >> 48) == RW_UNKNOWN);
            const int starts = len - n;
            for (int j = 0; j < starts; ++j) {
                bool eq = sh_key[(n << 7) + j] == key;
                if (eq && unk)
                    for (int q = 0; q <= n; ++q) eq = eq && sh_tok[i + q] == sh_tok[j + q];
                cnt += eq ? 1 : 0;
                first = first && !(eq && j < i);
            }
        }
        sh_tf[s] = (key && first) ? cnt : 0;
    }
    __syncthreads();

    // ---- pass 3: hypothesis tf-idf and norms; BLEU clipped counts; the closest reference length
    const int b0 = T.clip_bleu_ptr[c], b1 = T.clip_bleu_ptr[c + 1];
    double sq[2];
    int corr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * RW_THREADS;
        const int tf = sh_tf[s];
        double x = 0.0;
        int cc = 0;
        if (tf) {
            const uint64_t key = sh_key[s];
            const int g = T.n_global > 0 ? rw_find(T.g_keys, 0, T.n_global, key) : -1;
            x = (double)tf * (g >= 0 ? T.g_idf[g] : T.ref_len);
            const int m = rw_find(T.bleu_keys, b0, b1, key);
            if (m >= 0) { const int mc = T.bleu_cnt[m]; cc = mc < tf ? mc : tf; }
        }
        sh_x[s] = x;
        sq[h] = rw_wave_sum(x * x);
        corr[h] = rw_wave_sum_i(cc);
    }
    if (lane == 0) { sh_sq[wave][0] = sq[0]; sh_sq[wave][1] = sq[1]; sh_correct[wave][0] = corr[0]; sh_correct[wave][1] = corr[1]; }
    for (int q = ref0 + tid; q < ref1; q += RW_THREADS) {
        const int l = T.ref_tokens[q];
        const unsigned d = (unsigned)(l > len ? l - len : len - l);
        atomicMin(&sh_closest, ((unsigned long long)d << 32) | (unsigned)l);          // integer: (distance, length), ties to the shorter
    }
    __syncthreads();
    // slots 0..127 (n = 1) belong to waves 0, 1 at h = 0; 128..255 (n = 2) to waves 2, 3 at h = 0; n = 3, 4 the same at h = 1
    if (tid < 4) sh_norm[tid] = sqrt(sh_sq[(tid & 1) * 2][tid >> 1] + sh_sq[(tid & 1) * 2 + 1][tid >> 1]);
    __syncthreads();

    // ---- pass 4: CIDEr-D against every reference of the clip
    const uint64_t* rkeys = staged ? sh_rkey : T.ref_keys + k0;
    const double* rvals = staged ? sh_rval : T.ref_vals + k0;
    const int lh = len > 1 ? len - 1 : 0;                  // the hypothesis' bigram count: the reference's "length"
    double score[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = ref0 + wave; q < ref1; q += RW_WAVES) {
        const int lo = T.ref_key_ptr[q] - k0, hi = T.ref_key_ptr[q + 1] - k0;
        double val[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = lane + 64 * k;
            if (sh_tf[s]) {
                const int m = rw_find(rkeys, lo, hi, sh_key[s]);
                if (m >= 0) {
                    const double x = sh_x[s], y = rvals[m];
                    val[k >> 1] += (x < y ? x : y) * y;
                }
            }
        }
        const double delta = (double)(lh - T.ref_bigrams[q]);
        const double pen = exp(-(delta * delta) / (2.0 * 6.0 * 6.0));
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            double v = rw_wave_sum(val[n]);
            const double nh = sh_norm[n], nr = T.ref_norm[(int64_t)q * 4 + n];
            if (nh != 0.0 && nr != 0.0) v /= nh * nr;
            score[n] += v * pen;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) sh_score[wave][n] = score[n];
    }
    __syncthreads();

    // ---- pass 5: combine
    if (tid == 0) {
        double sum = 0.0;
#pragma unroll
        for (int n = 0; n < 4; ++n) sum += (sh_score[0][n] + sh_score[1][n]) + (sh_score[2][n] + sh_score[3][n]);
        const double cid = sum / 4.0 / (double)(ref1 - ref0) * 10.0;
        const int correct[4] = {sh_correct[0][0] + sh_correct[1][0], sh_correct[2][0] + sh_correct[3][0], sh_correct[0][1] + sh_correct[1][1],
                                sh_correct[2][1] + sh_correct[3][1]};
        double b = 1.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) b *= ((double)correct[k] + 1e-15) / ((double)(len - k > 0 ? len - k : 0) + 1e-9);
        b = pow(b, 0.25);
        const double reflen = (double)(unsigned)(sh_closest & 0xffffffffull);
        const double ratio = ((double)len + 1e-15) / (reflen + 1e-9);
        if (ratio < 1.0) b *= exp(1.0 - 1.0 / ratio);
        reward[r] = cid + b;
        if (cider) cider[r] = cid;
        if (bleu) bleu[r] = b;
    }
}

extern "C" int valor_caption_reward(void* stream, const int64_t* seq, int64_t ld, int R, int L, int64_t eos, int vocab, const int32_t* clip_idx,
                                    const RewardTables* tables, double* reward, double* cider, double* bleu) {
    if (R < 0 || L < 1 || L > RW_MAXL || vocab < 1 || vocab > 65534 || eos < 0 || eos >= vocab || ld < L) return VALOR_ERR_ARG;
    if (R == 0) return VALOR_OK;
    if (!seq || !clip_idx || !tables || !reward) return VALOR_ERR_ARG;
    const RewardTables& t = *tables;
    if (!t.clip_ref_ptr || !t.ref_key_ptr || !t.ref_keys || !t.ref_vals || !t.ref_norm || !t.ref_bigrams || !t.ref_tokens || !t.clip_bleu_ptr ||
        !t.bleu_keys || !t.bleu_cnt)
        return VALOR_ERR_ARG;
    if (t.n_clips < 1 || t.n_global < 0 || (t.n_global > 0 && (!t.g_keys || !t.g_idf))) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(caption_reward_kernel, dim3(R), dim3(RW_THREADS), 0, (hipStream_t)stream, seq, ld, L, eos, vocab, clip_idx, t, reward, cider,
                       bleu);
    return valor_launch_status();
}
