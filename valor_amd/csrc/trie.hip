// Closed answer sets at one decoding step (valor_trie_constrain; the law: include/valor_hip.h): every column of a row's fp32 logits that
// does not continue one of the candidates from the row's own generated tokens becomes VALOR_TRIE_FLOOR, in place. One launch between the
// decoding step and the selection, outside the captured step like valor_logits_constrain, with that kernel's history addressing
// (hist + (r % b) * hist_stride_s + (r / b) * hist_stride_k, sample s = r % b).
//   One 256-thread workgroup per row.
//   1. the history (t <= 512 ids) is copied to LDS by all four waves;
//   2. wave 0 walks the trie: per token a 64-way search of the node's ascending child list -- lane i probes element lo + i * stride, a
//      ballot counts the probes <= the token and names the stride that can hold it; a list of <= 64 children is one probe per lane and
//      one ballot. A root's few thousand children take two rounds, a node of the deeper levels one. Everything the walk leaves (node,
//      the child range, whether [SEP] is open) is wave-uniform and goes through four LDS words to the other waves;
//   3. the node's child tokens are copied to LDS when there are at most TRIE_LDS_CHILDREN of them (the 3129-answer root fits); a longer
//      list is searched where it lies, in global memory (L2-resident: every row reads the same few KiB);
//   4. the row is NOT read: a thread owns groups of four consecutive columns, a lower-bound search of the child list tells whether any
//      of the four is allowed; when none is -- all but a handful of the V / 4 groups -- one 16-byte store writes four floors, otherwise the
//      columns outside the set get single stores. Allowed columns, the pad behind V and inactive rows are never written, so they keep
//      their bits. When the base or the pitch is not a multiple of 16 bytes (ld = V = 30522 rows of the re-run path) the same loop runs
//      with groups of one column.
//   Every column is decided by the thread that owns it from the child list alone: no atomics, no workspace, nothing depends on how the
//   threads split the row. Indices are checked before they are used: a root or child outside [0, n_nodes) is "off the trie", a child
//   range is clamped to [0, n_edges].
#include "common.h"
#include "../../include/valor_hip.h"

#define TRIE_THREADS 256
#define TRIE_MAX_T 512
#define TRIE_LDS_CHILDREN 4096

// first index in [0, n) whose token is >= w (n when there is none); toks ascending
DEVINL int trie_lower_bound(const int32_t* toks, int n, int w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (toks[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the child of the range [lo, hi) whose token equals h, by wave 0 (all 64 lanes, uniform arguments and result): the edge index or -1
DEVINL int trie_find_child(const int32_t* __restrict__ child_tok, int lo, int hi, int64_t h, int lane) {
    while (hi - lo > WAVE) {
        const int stride = (hi - lo + WAVE - 1) / WAVE;
        const int p = lo + lane * stride;                                  // (< hi + stride <= 2^31: n_edges is an int)
        const bool le = p < hi && (int64_t)child_tok[p] <= h;
        const int cnt = __popcll(__ballot(le));                             // ascending: the lanes that hold are a prefix
        if (cnt == 0) return -1;
        lo += (cnt - 1) * stride;
        hi = min(lo + stride, hi);
    }
    const int p = lo + lane;
    const bool eq = p < hi && (int64_t)child_tok[p] == h;
    const unsigned long long m = __ballot(eq);
    return m ? lo + __ffsll((long long)m) - 1 : -1;
}

template <int G>
DEVINL void trie_mask_row(float* __restrict__ z, int V, const int32_t* toks, int n, int eos_open, int tid) {
    const int first = n ? toks[0] : 0, last = n ? toks[n - 1] : -1;
    for (int w0 = tid * G; w0 < V; w0 += TRIE_THREADS * G) {
        const int w1 = min(w0 + G, V);                                      // the group's columns [w0, w1)
        int pos = n;
        if (w1 > first && w0 <= last) pos = trie_lower_bound(toks, n, w0);
        const bool any = (pos < n && toks[pos] < w1) || (eos_open >= w0 && eos_open < w1);
        if (G == 4 && !any && w1 - w0 == 4) {
            const f32x4_t f = {VALOR_TRIE_FLOOR, VALOR_TRIE_FLOOR, VALOR_TRIE_FLOOR, VALOR_TRIE_FLOOR};
            *(f32x4_t*)(z + w0) = f;
            continue;
        }
        for (int w = w0; w < w1; ++w) {
            while (pos < n && toks[pos] < w) ++pos;
            const bool in = (pos < n && toks[pos] == w) || w == eos_open;
            if (!in) z[w] = VALOR_TRIE_FLOOR;
        }
    }
}

__global__ __launch_bounds__(TRIE_THREADS) void trie_constrain_kernel(float* __restrict__ logits, int64_t ld, int V,
                                                                     const int64_t* __restrict__ hist, int64_t hist_stride_s,
                                                                     int64_t hist_stride_k, int b, int t, int eos,
                                                                     const int32_t* __restrict__ child_ptr,
                                                                     const int32_t* __restrict__ child_tok,
                                                                     const int32_t* __restrict__ child_node,
                                                                     const uint8_t* __restrict__ terminal, const int32_t* __restrict__ root,
                                                                     int n_nodes, int n_edges, int n_roots, const uint8_t* __restrict__ active,
                                                                     int vec) {
    __shared__ int64_t h[TRIE_MAX_T];
    __shared__ int32_t kids[TRIE_LDS_CHILDREN];
    __shared__ int walk[4];                                                  // child range lo, hi; [SEP] open
    const int r = blockIdx.x, tid = threadIdx.x;
    if (active && !active[r]) return;                                        // (workgroup-uniform)
    if (t > 0) {
        const int64_t* src = hist + (int64_t)(r % b) * hist_stride_s + (int64_t)(r / b) * hist_stride_k;
        for (int i = tid; i < t; i += TRIE_THREADS) h[i] = src[i];
    }
    __syncthreads();
    if (tid < WAVE) {
        int node = root[n_roots == 1 ? 0 : r % b];
        if (node < 0 || node >= n_nodes) node = -1;
        int lo = 0, hi = 0;
        for (int i = 0; i <= t; ++i) {                                       // the node's child range, then the step along token i
            lo = hi = 0;
            if (node < 0) break;
            lo = min(max(child_ptr[node], 0), n_edges);
            hi = min(max(child_ptr[node + 1], lo), n_edges);
            if (i == t) break;
            const int e = trie_find_child(child_tok, lo, hi, h[i], tid);
            node = e < 0 ? -1 : child_node[e];
            if (node < 0 || node >= n_nodes) node = -1;
        }
        if (tid == 0) {
            walk[0] = lo;
            walk[1] = hi;
            walk[2] = (node < 0 || terminal[node]) ? eos : -1;
        }
    }
    __syncthreads();
    const int lo = walk[0], n = walk[1] - walk[0], eos_open = walk[2];
    const int32_t* toks = child_tok + lo;
    if (n <= TRIE_LDS_CHILDREN) {
        for (int i = tid; i < n; i += TRIE_THREADS) kids[i] = toks[i];
        __syncthreads();                                                     // (n is workgroup-uniform)
        toks = kids;
    }
    float* z = logits + (int64_t)r * ld;
    if (vec) trie_mask_row<4>(z, V, toks, n, eos_open, tid);
    else trie_mask_row<1>(z, V, toks, n, eos_open, tid);
}

extern "C" int valor_trie_constrain(void* stream, float* logits, int64_t ld, int R, int V, const int64_t* hist, int64_t hist_stride_s,
                                    int64_t hist_stride_k, int b, int t, int64_t eos, const int32_t* child_ptr, const int32_t* child_tok,
                                    const int32_t* child_node, const uint8_t* terminal, const int32_t* root, int n_nodes, int n_edges,
                                    int n_roots, const uint8_t* active) {
    if (R == 0) return VALOR_OK;
    if (!logits || R < 0 || V < 1 || ld < V || t < 0 || t > TRIE_MAX_T || (!hist && t > 0)) return VALOR_ERR_ARG;
    if (b < 1 || hist_stride_s < 0 || hist_stride_k < 0 || eos < 0 || eos >= V) return VALOR_ERR_ARG;
    if (!child_ptr || !terminal || !root || n_nodes < 1 || n_edges < 0 || ((!child_tok || !child_node) && n_edges > 0)) return VALOR_ERR_ARG;
    if (n_roots != 1 && n_roots != b) return VALOR_ERR_ARG;
    const int vec = ((uintptr_t)logits % 16 == 0 && ld % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(trie_constrain_kernel, dim3(R), dim3(TRIE_THREADS), 0, (hipStream_t)stream, logits, ld, V, hist, hist_stride_s,
                       hist_stride_k, b, t, (int)eos, child_ptr, child_tok, child_node, terminal, root, n_nodes, n_edges, n_roots, active, vec);
    return valor_launch_status();
}

// ------------------------------------------------------------------------------------------
// Exact ranking of a whole closed answer set, one trie level per launch (valor_trie_score_level; the law: include/valor_hip.h). Row
// r = i * b + s of the fp32 logits is the decoder's output for node level_node[i] and sample s: the row scores ALL of the node's children
// and its own end-of-answer term, so a candidate's sequence log-probability costs one decoder row per trie NODE instead of one per
// (candidate, step).
//   One 256-thread workgroup per row.
//   1. lse given: the row is not streamed at all, only the node's columns are gathered. lse null: one pass over the row's V floats --
//      16-byte loads (four in flight per thread) when the base and the pitch allow, 4-byte loads otherwise -- with a running
//      (maximum, sum of exp) pair per thread; the 256 pairs meet in fp64 (wave shuffles, four LDS words) and the logarithm is taken in
//      fp64, so lse_r carries one fp32 rounding besides the error of the fp32 partial sums.
//   2. the threads stride over the node's edges: node_score[child] = node_score[node] + (z[tok] - lse_r), the subtraction rounded first;
//      thread 0 adds the [SEP] term of a terminal node into final[node]. The gathered columns were just streamed: they come out of L2.
//   Every output element is written once by the thread that owns its edge: no atomics, no workspace, no LDS beyond the reduction words;
//   the logits are read-only. A level_node / child_node outside [0, n_nodes) or a child token outside [0, V) is never dereferenced: the
//   row / edge writes nothing. A child range is clamped to [0, n_edges].
DEVINL double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

DEVINL void tsl_fold(float& m, float& s, float z) {
    if (z > m) { s *= expf(m - z); m = z; }                                  // (m = -inf: s is 0 and stays 0)
    s += expf(z - m);
}

DEVINL void tsl_fold4(float& m, float& s, const f32x4_t v) {
    const float vm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (vm > m) { s *= expf(m - vm); m = vm; }
    s += (expf(v[0] - m) + expf(v[1] - m)) + (expf(v[2] - m) + expf(v[3] - m));
}

__global__ __launch_bounds__(TRIE_THREADS) void trie_score_level_kernel(const float* __restrict__ logits, int64_t ld, int V, int b,
                                                                       const int32_t* __restrict__ level_node,
                                                                       const float* __restrict__ lse, float* __restrict__ lse_out, int eos,
                                                                       const int32_t* __restrict__ child_ptr,
                                                                       const int32_t* __restrict__ child_tok,
                                                                       const int32_t* __restrict__ child_node,
                                                                       const uint8_t* __restrict__ terminal, int n_nodes, int n_edges,
                                                                       float* __restrict__ node_score, float* __restrict__ final, int vec) {
    __shared__ float red_m[4];
    __shared__ double red_s[4];
    __shared__ float row_lse;
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = (int)(r % b);
    const float* z = logits + r * ld;
    float l;
    if (lse) {
        l = lse[r];
    } else {
        float m = -INFINITY, acc = 0.f;
        if (vec) {
            const int V4 = V & ~3;
            for (int j0 = tid * 4; j0 < V4; j0 += 4 * 4 * TRIE_THREADS) {
                f32x4_t v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * 4 * TRIE_THREADS;
                    if (j < V4) v[u] = *(const f32x4_t*)(z + j);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j0 + u * 4 * TRIE_THREADS < V4) tsl_fold4(m, acc, v[u]);
            }
            if (V4 + tid < V) tsl_fold(m, acc, z[V4 + tid]);
        } else {
            for (int j = tid; j < V; j += TRIE_THREADS) tsl_fold(m, acc, z[j]);
        }
        const float wm = wave_max(m);
        if (lane == 0) red_m[wave] = wm;
        __syncthreads();
        const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        const double part = wave_sum_f64(m == -INFINITY ? 0.0 : (double)acc * (double)expf(m - M));
        if (lane == 0) red_s[wave] = part;
        __syncthreads();
        if (tid == 0) {
            const float v = (float)((double)M + log((red_s[0] + red_s[1]) + (red_s[2] + red_s[3])));
            row_lse = v;
            if (lse_out) lse_out[r] = v;
        }
        __syncthreads();
        l = row_lse;
    }
    const int node = level_node[r / b];
    if (node < 0 || node >= n_nodes) return;                                 // (workgroup-uniform)
    const float own = node_score[(int64_t)node * b + s];
    const int lo = min(max(child_ptr[node], 0), n_edges);
    const int hi = min(max(child_ptr[node + 1], lo), n_edges);
    for (int e = lo + tid; e < hi; e += TRIE_THREADS) {
        const int w = child_tok[e], c = child_node[e];
        if (w < 0 || w >= V || c < 0 || c >= n_nodes) continue;
        const float term = z[w] - l;
        node_score[(int64_t)c * b + s] = own + term;
    }
    if (tid == 0 && terminal[node]) {
        const float term = z[eos] - l;
        final[(int64_t)node * b + s] = own + term;
    }
}

extern "C" int valor_trie_score_level(void* stream, const float* logits, int64_t ld, int64_t rows, int V, int b, const int32_t* level_node,
                                      const float* lse, float* lse_out, int64_t eos, const int32_t* child_ptr, const int32_t* child_tok,
                                      const int32_t* child_node, const uint8_t* terminal, int n_nodes, int n_edges, float* node_score,
                                      float* final) {
    if (rows == 0) return VALOR_OK;
    if (!logits || !level_node || !child_ptr || !terminal || !node_score || !final) return VALOR_ERR_ARG;
    if (rows < 0 || rows > 0x7fffffffll || V < 1 || ld < V || b < 1 || rows % b != 0 || eos < 0 || eos >= V) return VALOR_ERR_ARG;
    if (n_nodes < 1 || n_edges < 0 || rows / b > n_nodes || ((!child_tok || !child_node) && n_edges > 0)) return VALOR_ERR_ARG;
    const int vec = ((uintptr_t)logits % 16 == 0 && ld % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(trie_score_level_kernel, dim3((unsigned)rows), dim3(TRIE_THREADS), 0, (hipStream_t)stream, logits, ld, V, b, level_node,
                       lse, lse_out, (int)eos, child_ptr, child_tok, child_node, terminal, n_nodes, n_edges, node_score, final, vec);
    return valor_launch_status();
}
