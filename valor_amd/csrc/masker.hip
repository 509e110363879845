// Device-side BERT token masking (model/modeling.py:134-174) and the masked-row gather table of the decoder passes
// (pretrain.py:441,495). The host draws how MANY positions each row masks (k_i ~ Binomial(m_i, p) | k_i >= 1, valor_amd/model/valor.py
// DeviceTokenMasker); these kernels decide WHICH, and what the selected positions become:
//   - every candidate (j >= 1, token != 0) of row i draws Philox4x32-10(seed, offset + i*T + j); words 0-1 are its 64-bit key
//     (w0 | w1 << 32); the row keeps the k_i candidates with the smallest keys, ties broken by position. The k-smallest-keys subset
//     of i.i.d. keys is uniform over the k-subsets, so count + subset has the reference's joint law;
//   - word 2 against floor(0.8 * 2^32) / floor(0.9 * 2^32): [MASK] / a random token / the token kept (80 / 10 / 10 %);
//   - word 3 picks the random token as range_start + umulhi(w3, range_end - range_start). Over R = range_end - range_start values
//     a value is hit by floor(2^32 / R) or that + 1 of the 2^32 words: relative bias below R / 2^32, i.e. below 2^-17 for the BERT
//     vocabulary's R = 30522 - 106.
// One wave per row, nothing atomic: the outputs are a function of (tokens, k, seed, offset) alone.
#include "common.h"

#define MASK_MAX_T 512                         // the BERT position table (bert.py:195)
#define MASK_THR_MASK 3435973836u              // floor(0.8 * 2^32)
#define MASK_THR_RANDOM 3865470566u            // floor(0.9 * 2^32)

DEVINL uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// grid = b blocks of one wave. Pass 1 writes the row's candidate keys into LDS in position order (ballot + popcount prefix); pass 2
// ranks each candidate by a count over the row and writes every position of tokens_out / labels.
__global__ __launch_bounds__(64) void mask_tokens_kernel(const int64_t* __restrict__ tokens, const int32_t* __restrict__ k, int T,
                                                         uint64_t seed, uint64_t offset, int64_t mask_token, int64_t range_start,
                                                         uint32_t range_n, int64_t* __restrict__ tokens_out, int64_t* __restrict__ labels) {
    __shared__ uint64_t keys[MASK_MAX_T];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int64_t* row = tokens + (int64_t)i * T;
    const uint64_t ctr0 = offset + (uint64_t)i * (uint64_t)T;
    int m = 0;
    for (int c = 0; c < T; c += WAVE) {
        const int j = c + lane;
        const bool cand = j >= 1 && j < T && row[j] != 0;
        const uint64_t bal = __ballot(cand);
        if (cand) {
            const Philox4 r = philox4x32_10(seed, ctr0 + j);
            keys[m + __popcll(bal & lanes_below(lane))] = (uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32);
        }
        m += __popcll(bal);
    }
    __syncthreads();
    const int ki = min(max(k[i], 0), m);       // the host guarantees 1 <= k_i <= m_i; a bad k cannot select more than the row has
    int base = 0;
    for (int c = 0; c < T; c += WAVE) {
        const int j = c + lane;
        const int64_t t = j < T ? row[j] : 0;
        const bool cand = j >= 1 && j < T && t != 0;
        const uint64_t bal = __ballot(cand);
        int64_t o = t, lab = -1;
        if (cand) {
            const int slot = base + __popcll(bal & lanes_below(lane));
            const uint64_t key = keys[slot];
            int rank = 0;
            for (int q = 0; q < m; ++q) {
                const uint64_t kq = keys[q];
                rank += (kq < key) | ((kq == key) & (q < slot));
            }
            if (rank < ki) {
                const Philox4 r = philox4x32_10(seed, ctr0 + j);
                lab = t;
                if (r.v[2] < MASK_THR_MASK) o = mask_token;
                else if (r.v[2] < MASK_THR_RANDOM) o = range_start + (int64_t)__umulhi(r.v[3], range_n);
            }
        }
        base += __popcll(bal);
        if (j < T) {
            tokens_out[(int64_t)i * T + j] = o;
            labels[(int64_t)i * T + j] = lab;
        }
    }
}

// grid = b blocks of one wave. Row i's selected positions (label != -1), in position order, go to slots row_off[i] + 0, 1, ... of every
// group g: idx[g*n + s] = r0 + (g*b + i)*Ttot + j, lab_out[g*n + s] = label. A row writes only inside [row_off[i], row_off[i + 1])
// (row_off[b] = n), so labels that disagree with the offsets cannot write out of range.
__global__ __launch_bounds__(64) void masked_rows_kernel(const int64_t* __restrict__ labels, const int32_t* __restrict__ row_off, int b, int T,
                                                         int G, int64_t Ttot, int64_t r0, int64_t n, int64_t* __restrict__ idx,
                                                         int64_t* __restrict__ lab_out) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int64_t off = row_off[i];
    const int64_t end = min(i + 1 < b ? (int64_t)row_off[i + 1] : n, n);
    const int64_t cap = off < 0 ? 0 : end - off;
    const int64_t* row = labels + (int64_t)i * T;
    int64_t base = 0;
    for (int c = 0; c < T; c += WAVE) {
        const int j = c + lane;
        const int64_t lab = j < T ? row[j] : -1;
        const bool sel = lab != -1;
        const uint64_t bal = __ballot(sel);
        const int64_t s = base + __popcll(bal & lanes_below(lane));
        if (sel && s < cap) {
            for (int g = 0; g < G; ++g) {
                idx[g * n + off + s] = r0 + ((int64_t)g * b + i) * Ttot + j;
                lab_out[g * n + off + s] = lab;
            }
        }
        base += __popcll(bal);
    }
}

extern "C" int valor_mask_tokens(void* stream, const int64_t* tokens, const int32_t* k, int b, int T, uint64_t seed, uint64_t offset,
                                 int64_t mask_token, int64_t range_start, int64_t range_end, int64_t* tokens_out, int64_t* labels) {
    if (!tokens || !k || !tokens_out || !labels) return VALOR_ERR_ARG;
    if (b <= 0 || T <= 0 || T > MASK_MAX_T) return VALOR_ERR_ARG;
    if (range_start < 0 || range_end <= range_start || range_end - range_start > 0xffffffffll) return VALOR_ERR_ARG;
    hipLaunchKernelGGL(mask_tokens_kernel, dim3(b), dim3(WAVE), 0, (hipStream_t)stream, tokens, k, T, seed, offset, mask_token, range_start,
                       (uint32_t)(range_end - range_start), tokens_out, labels);
    return valor_launch_status();
}

extern "C" int valor_masked_rows(void* stream, const int64_t* labels, const int32_t* row_off, int b, int T, int G, int64_t Ttot, int64_t r0,
                                 int64_t n, int64_t* idx, int64_t* lab_out) {
    if (!labels || !row_off || !idx || !lab_out) return VALOR_ERR_ARG;
    if (b <= 0 || G <= 0 || T <= 0 || T > MASK_MAX_T || Ttot < T || r0 < 0 || n < 0) return VALOR_ERR_ARG;
    if (n == 0) return VALOR_OK;
    hipLaunchKernelGGL(masked_rows_kernel, dim3(b), dim3(WAVE), 0, (hipStream_t)stream, labels, row_off, b, T, G, Ttot, r0, n, idx, lab_out);
    return valor_launch_status();
}
