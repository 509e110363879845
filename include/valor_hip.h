/* valor_hip.h -- C ABI of libvalor_hip.so: the MI355X (gfx950) kernels of the VALOR pretraining step.
 *
 * The reference (TXH-mercury/VALOR) has no native plugin ABI for this path: its only native boundary is the
 * pybind module of apex's FusedLayerNorm (apex/csrc/layer_norm_cuda.cpp:235-240, at::Tensor arguments) and
 * amp_C (apex/csrc/amp_C_frontend.cpp:116-134); everything else is torch ops called from Python
 * (model/pretrain.py, model/modeling.py, model/bert.py, model/clip.py, model/transformer.py, optim/adamw.py).
 * This header DEFINES the boundary a maintainer binds instead (ctypes / pybind / cgo alike): plain C, raw
 * device pointers, sizes and strides -- no torch types. Each entry cites the reference code it replaces.
 *
 * Conventions
 *   - every function is asynchronous on `stream` (a hipStream_t passed as void*), returns 0 on success,
 *     VALOR_ERR_ARG (-1) on a bad argument, VALOR_ERR_LAUNCH (-2) if the launch failed; nothing throws;
 *   - the caller owns all memory (kernels never allocate); workspaces are explicit arguments;
 *   - dtype: VALOR_DT_BF16 (0) = bf16 storage / fp32 accumulate (perf mode), VALOR_DT_F32 (1) = fp32 storage,
 *     exact fp32 MFMA (parity mode). Pointers typed `void*` hold elements of `dtype`;
 *   - all compute entry points are re-entrant (autograd may call from a worker thread) and keep no state between calls.
 *     The ONLY process-global state is the kernel-family selection of the tuning hooks (valor_gemm_set_variant,
 *     valor_gemm_set_policy, valor_gemm_set_tr_asm, valor_gemm_set_fast_epilogue, valor_attn_set_variant,
 *     valor_attn_set_res_pipeline, valor_win_attn_set_variant, valor_ln_set_variant, valor_ln_set_nt, valor_adamw_set_nt,
 *     valor_fine_set_fused and their VALOR_* environment presets): plain ints read at launch time, every setting selects a
 *     parity-tested kernel family computing the same function, so a concurrent change can alter speed, never results beyond
 *     rounding.
 *   - dropout masks are Philox4x32-10 streams keyed by (seed, offset + element index / 4) and are regenerated
 *     in backward from the same (seed, offset) -- nothing is stored. Every dropout entry point also takes `rng_base`: NULL, or a
 *     DEVICE pointer to one uint64 that the kernel adds to `offset` when it runs (forward and backward of a step must see the same
 *     value). By-value arguments are baked into a captured hipGraph; with the device-resident term the caller bumps one counter
 *     per step (any kernel / memset node ahead of the step) and every replay of the graph draws fresh masks
 *     (train_utils.py:309: the reference advances torch's global generator once per dropout call).
 *     That Philox law is the one of the LayerNorm-side kernels (valor_bdrln_*): element (row, c) of a [rows, cols] operand reads word
 *     c % 4 of Philox4x32-10(seed, offset + (row * cols + c) / 4) and is KEPT iff word >= drop_threshold(p) = (uint32)((double)p * 2^32).
 *     The attention kernels (valor_attn_fwd / valor_attn_bwd, valor_cross_attn_*_fused) draw one 32-bit hash per probability instead
 *     (csrc/attn_common.h), with the same threshold and the same 64-bit offset = `offset` + *rng_base:
 *         hk   = attn_drop_headkey(seed, offset, b * H + h)     b: the QUERY batch (also under kv_bmod), h: the head
 *                = mix32(mix32(mix32(lo32(offset) + (b * H + h) * 0x9E3779B9) ^ hi32(offset) ^ lo32(seed)) + hi32(seed))
 *         bits = attn_drop_bits(hk, q * Skv + j)                q: query row, j: key index LOCAL to the batch's kv_range (j = key - start),
 *                                                               Skv: the launch's K / V rows per batch (the pitch, never the range length)
 *                = x ^ (x >> 13),  x = mul24(y ^ (y >> 15), 0x85EBCB) + hk,  y = mul24(j' ^ hk, 0x9E3779) + (hk >> 7),  j' = q * Skv + j
 *         (mix32: x ^= x >> 16, x *= 0x7FEB352D, x ^= x >> 15, x *= 0x846CA68B, x ^= x >> 16; mul24: low 24 bits of both operands, low 32 of
 *         the product; all arithmetic modulo 2^32). P[q, j] is kept iff bits >= drop_threshold(p), kept values are scaled by 1 / (1 - p),
 *         lse is of the undropped scores. Sq * Skv must stay below 2^24 (checked). tests/dropout_ref.py restates both laws on the host.
 */
#ifndef VALOR_HIP_H
#define VALOR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VALOR_DT_BF16 0
#define VALOR_DT_F32 1
#define VALOR_OK 0
#define VALOR_ERR_ARG (-1)
#define VALOR_ERR_LAUNCH (-2)
/* activations of the GEMM epilogue */
#define VALOR_ACT_NONE 0
#define VALOR_ACT_GELU_ERF 1   /* bert.py:52-57, transformer.py:32-38 */
#define VALOR_ACT_QUICK_GELU 2 /* clip.py:167-169 */
#define VALOR_ACT_RELU 3       /* pretrain.py:104-112 */
#define VALOR_ACT_TANH 4
/* OR-ed onto an activation id: `preact` of the forward GEMM receives act'(x) instead of x, and `dact_aux` of the matching dgrad
 * holds that derivative (the epilogue multiplies by it: no sigmoid / erf / exp in the backward). The autograd contract of
 * nn.Linear + activation is unchanged; only what is kept between forward and backward differs. */
#define VALOR_ACT_DERIV 16

/* ---- GEMM: C[M,N] = epi(alpha * op(A)[M,K] . op(B)[N,K]^T).  Replaces every nn.Linear / matmul projection and its
 * autograd GEMMs: bert.py:233-235,245-247,303-305,352,366,404,417; clip.py:176-182,237,329; transformer.py:109-142;
 * modeling.py:249-253; pretrain.py:36-38,90-91.  transX=0: X(row,k)=X[row*ldx+k]; transX=1: X(row,k)=X[k*ldx+row].
 * epilogue: + bias[N]; optional copy of the pre-activation to `preact`; act; or multiply by act'(dact_aux) (backward of a
 * fused activation); C += result when `accumulate`; out_f32 stores C/preact as fp32 for bf16 inputs.
 * workspace: fp32 scratch for split-K partial tiles (may be NULL = no split-K).
 * rowsum_out (may be NULL): [M] values of C's element type, the sums over k of op(A) -- the bias gradient of a wgrad GEMM (sum over tokens of dY) computed on
 * the matrix pipe beside the GEMM instead of a separate pass over dY; only where valor_gemm_kernel_for() returns 3 or 4 and
 * transA = 1 (VALOR_ERR_ARG otherwise). */
int valor_gemm(void* stream, int dtype, int transA, int transB, int M, int N, int K, const void* A, int64_t lda,
               const void* B, int64_t ldb, void* C, int64_t ldc, const void* bias, int act, void* preact,
               const void* dact_aux, int64_t ldaux, float alpha, int accumulate, int out_f32, void* workspace,
               int64_t workspace_bytes, void* rowsum_out,
               int rowsum_accumulate);

/* ---- per-call tuning. The valor_gemm_set_* hooks above change PROCESS defaults (A/B tooling, env presets). A caller that wants a
 * kernel choice for ONE call -- without touching state other threads read -- passes a valor_gemm_policy: every field is the value
 * the corresponding hook would set, -1 = keep the process default. valor_gemm_tuned(policy, ...) = valor_gemm(...) under that policy,
 * valor_gemm_kernel_for_tuned reports the family it would pick. (policy = NULL: exactly valor_gemm / valor_gemm_kernel_for.) */
typedef struct valor_gemm_policy {
    int key[12];        /* valor_gemm_set_policy keys 0 .. 11 */
    int variant;        /* valor_gemm_set_variant */
    int tr_asm;         /* valor_gemm_set_tr_asm */
    int fast_epilogue;  /* valor_gemm_set_fast_epilogue */
    int sched_256;      /* valor_gemm_set_8ph_sched */
    int sched_narrow;   /* valor_gemm_set_narrow_sched */
} valor_gemm_policy;
int valor_gemm_tuned(const valor_gemm_policy* policy, void* stream, int dtype, int transA, int transB, int M, int N, int K,
                     const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const void* bias, int act,
                     void* preact, const void* dact_aux, int64_t ldaux, float alpha, int accumulate, int out_f32, void* workspace,
                     int64_t workspace_bytes, void* rowsum_out, int rowsum_accumulate);
int valor_gemm_kernel_for_tuned(const valor_gemm_policy* policy, int dtype, int transA, int transB, int M, int N, int K,
                                int heavy_epilogue);

/* ---- split-K reductions deferred and grouped. The wgrad GEMMs of a layer (bert.py:233-235,352,366,404,417; clip.py:176-182) are each
 * split along the token contraction and each ends in a small reduction launch -- 309 of them per VALOR-base step. valor_gemm_deferred
 * is valor_gemm except that, when the product is split, the partial tiles stay in the caller's workspace PIECE (one piece per pending
 * product, untouched until the group reduction has been enqueued on the same stream) and `pending` (host memory) receives what is
 * left to do; valor_gemm_pending_bytes stores how much of the piece is occupied (0: the product was not split and is complete);
 * valor_gemm_reduce_group sums the partials of up to 8 pending products of one dtype and applies their epilogues (alpha, bias,
 * C +=, fused row sums) in ONE launch. Per element the arithmetic is that of valor_gemm's own reduction: bit-identical results. */
typedef struct valor_gemm_pending { unsigned char opaque[256]; } valor_gemm_pending;
int valor_gemm_deferred(void* stream, int dtype, int transA, int transB, int M, int N, int K, const void* A, int64_t lda,
                        const void* B, int64_t ldb, void* C, int64_t ldc, const void* bias, int act, void* preact,
                        const void* dact_aux, int64_t ldaux, float alpha, int accumulate, int out_f32, void* workspace,
                        int64_t workspace_bytes, void* rowsum_out, int rowsum_accumulate, valor_gemm_pending* pending);
int valor_gemm_pending_bytes(const valor_gemm_pending* pending, int64_t* bytes);
int valor_gemm_reduce_group(void* stream, int dtype, const valor_gemm_pending* pendings, int n);

/* ---- the weight gradients of a layer as ONE grouped split-K launch. Launched alone, each short wgrad of an AST / decoder layer is split
 * until it fills a round of the 256 workgroup slots of the 256x256 kernel by itself: 7 .. 28 slices of 6 .. 37 K-tiles behind a full
 * prologue and a full partial-tile epilogue each. A layer's six products are independent: issued together they fill the round with two
 * slices (69 / 129 K-tiles per workgroup), a quarter of the partial-tile traffic and one ramp / tail instead of six.
 *   valor_gemm_group_problem describes one product in `blob` and launches nothing. It takes bf16  C += alpha A^T . B  (valor_gemm's
 *     transA = transB = 1, accumulate = 1, no bias / activation; rowsum_out as in valor_gemm) where valor_gemm_kernel_for answers 3,
 *     valor_gemm's own split would leave at most 48 K-tiles per workgroup (the ViT / cross-K|V wgrads run 225 and keep their launches)
 *     and no per-call policy is in force; anything else is VALOR_ERR_ARG and goes through valor_gemm / valor_gemm_deferred as before.
 *   valor_gemm_group(stream, dtype, blobs, n, workspace, workspace_bytes) issues the n <= 8 described products as one launch. Slice plan:
 *     the smallest common K-tile count per workgroup (>= 6) whose slice counts S_i = ceil(K_i / 64 / kt) fit sum tiles_i S_i <= 256; a
 *     group whose tiles exceed half a round runs unsplit and accumulates straight into C. Partial tiles (bf16 under policy key 1) and the
 *     [S][M] row-sum partials go to `workspace` (256-byte aligned; at most 65 MiB, VALOR_ERR_ARG if it does not fit), which stays
 *     untouched until valor_gemm_reduce_group(stream, dtype, blobs, n) -- the blobs leave here as its pending products -- is enqueued.
 *     Kernel: the four-wave loop of csrc/gemm8q.hip when the group's shortest K loop exceeds 48 K-tiles (policy key 12 = 0 / 1: never /
 *     always), else the eight-wave pipelined loop; inside a slice every accumulator receives its K-tiles in valor_gemm's order.
 *   valor_gemm_group_plan answers the plan for n shapes (M, N, K, fused row sums 0 / 1: 4 ints each) on the host: slices[n], ksteps[n]
 *     (either may be NULL), info[4] = work items, shortest K loop in K-tiles, 1 if csrc/gemm8q.hip would run it, workspace bytes / 256.
 * valor_amd queues eligible wgrads per stream and issues them at the end of the layer / of the backward pass (kernels.ReduceQueue;
 * env VALOR_GROUP_WGRAD). */
int valor_gemm_group_problem(valor_gemm_pending* blob, int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B,
                             int64_t ldb, void* C, int64_t ldc, float alpha, int accumulate, void* rowsum_out, int rowsum_accumulate);
int valor_gemm_group(void* stream, int dtype, valor_gemm_pending* blobs, int n, void* workspace, int64_t workspace_bytes);
int valor_gemm_group_plan(const int* shapes, int n, int* slices, int* ksteps, int* info);

/* selects the bf16 kernel of valor_gemm: 0 = register-staged 128x128 tiles, 1 = LDS-DMA (buffer_load ... lds) 128x128
 * single stage, 2 = LDS-DMA 128x128 double stage, 3 = 256x256 8-phase pipeline wherever eligible, 4 = measured per-shape
 * policy between 1 and 3 (default). Returns the previous value; v < 0 only queries. Tuning / A-B measurement hook. */
int valor_gemm_set_variant(int v);
/* kernel family valor_gemm picks for a problem under the current variant: 0 = register-staged 128x128 (and every fp32
 * problem), 1 / 2 = LDS-DMA 128x128 single / double stage, 3 = 256x256 8-phase (one workgroup per CU), 4 = 256x128 8-phase with
 * two workgroups per CU (csrc/gemm8n.hip, policy key 8) */
int valor_gemm_kernel_for(int dtype, int transA, int transB, int M, int N, int K, int heavy_epilogue);
/* heavy_epilogue: the call passes dact_aux WITHOUT VALOR_ACT_DERIV (the epilogue evaluates act' of a second [M, N] operand); such dgrads stay on the 128x128 kernel below
 * K = 1536, where four workgroups per CU overlap each other's epilogues (profiles/r02_gemm_epilogue_ab.json) */
/* k-slow 8-phase kernels: transposing LDS reads as inline asm (keeps the counted LDS-DMA pipeline from being drained by
 * compiler-inserted waits); returns the previous value, v < 0 only queries */
int valor_gemm_set_tr_asm(int v);
/* 8-phase kernels: bf16 tile epilogue (bias / activation on the accumulators, the 256 x 256 tile as bf16 through LDS once, twice
 * when a pre-activation copy is wanted; act' multiply and C += at read-out) for bf16 C without split-K / fused row sums, N % 8 == 0,
 * ldc % 8 == 0; default on. Returns the previous value, v < 0 only queries */
int valor_gemm_set_fast_epilogue(int v);
/* policy parameters of variant 4 and of the 8-phase launch (tuning / A-B hook; returns the previous value, value < 0 only queries):
 *   key 0: smallest K for which a big-M dgrad (A row-major, B k-slow) runs on the 256x256 8-phase kernel
 *   key 1: 1 = the split-K partial tiles of the bf16 LDS-DMA kernels are written and summed as bf16 (half the workspace traffic, one more
 *          rounding per partial; never for fp32 outputs); default 1 (in-step +1.3 %, profiles/r03_step_ab_s3.txt; error bound asserted in
 *          tests/test_gemm_bench_shapes_gpu.py::test_wgrad_splitk_with_bf16_partials)
 *   key 2: smallest number of 256x256 tiles for the 8-phase kernel on forward problems (default 256: one full round of workgroups)
 *   key 3: the same for dgrad problems (default 1024: below it the 128x128 kernel measured faster, session N)
 *   key 4: L2-aware tile raster of the 8-phase kernels: 0 = row-major over all tile columns; G > 0 = groups of G tile columns
 *          (each XCD keeps G weight panels of 256 x K in its 4 MiB L2 and streams the activation rows past them); 1000 (default) = G
 *          from a fabric-traffic model per problem (csrc/gemm8.hip launch_gemm_8ph). Measured with non-temporal stores: fabric traffic
 *          2.27 -> 1.54 x algorithmic on the ViT fc1 forward (profiles/r03_pmc_gemm_l2_v2_nt_stores.json), kernel time -1 .. +3 %,
 *          step +0.45 % (profiles/r03_step_ab_s3.txt)
 *   key 5: bf16 output stores of the 8-phase kernels: 0 plain, 1 non-temporal, 1000 (default) = non-temporal for K <= 1024
 *          (+5.5 .. +10 % on the K = 768 forward shapes, -0.6 .. -1.8 % at K = 3072)
 *   key 6: 1 = the 128x128 kernels store big outputs of short-K problems non-temporally too (default 0)
 *   key 7: smallest K of a forward (NN) problem that may use the 8-phase kernels (default 128, env VALOR_GEMM_NN_MINK)
 *   key 8: the 256x128 two-workgroups-per-CU 8-phase kernel (family 4; K % 64 == 0, K >= 128, M >= 256, N >= 128; env VALOR_GEMM_NARROW):
 *          0 = never, 1 = every eligible problem, 2 = only problems the keys above leave to the 128x128 kernels, 3 = only problems they
 *          send to the 256x256 kernel, 1000 (default) = measured per-class choice: forward / dgrad problems that
 *          would run on the 128x128 kernels or have K <= 1024
 *   key 9: family 4, NN layout (forward GEMMs): 1 = main loop on v_mfma_f32_32x32x16_bf16 (32-row fragments, another LDS swizzle; same
 *          results up to the order of the fp32 partial sums), 0 (default) = v_mfma_f32_16x16x32_bf16 (env VALOR_GEMM_MFMA32); measured
 *          0-8 % SLOWER on the K = 768 forward shapes under the pipelined schedule, equal under the plain one and at K = 3072
 *          (profiles/r05_gemm_mfma32_ab.json)
 *   key 10: family 4, NN layout without split-K: 1 = 512-thread workgroups of 64x64 wave tiles (csrc/gemm8w.hip; env VALOR_GEMM_WIDE), 0 (default):
 *          measured equal (profiles/r06_gemm_wide_ab_v2.json)
 *   key 11: the largest M of a few-row NN product that runs on the weight-streaming kernel (family 5, csrc/gemm_skinny.hip: K in {512, 768, 1024,
 *          3072, 4096}; plain / bias / activation / alpha / fp32-output epilogues -- a call that asks for C +=, a pre-activation copy or an
 *          act' operand runs on the 128x128 kernels): 0 = never = the process default (the training step keeps the kernels its parity evidence
 *          was collected on); the inference paths of valor_amd ask for 384 per call through a valor_gemm_policy (env VALOR_GEMM_SKINNY; env
 *          VALOR_GEMM_SKINNY_ALL sets the process default). nn.Linear on the 2 rows per sequence of a
 *          K|V-cached decoding step (model/bert.py:233-235,351,403-420): 20-29 us -> 8.8-17.6 us per launch
 *          (profiles/r06_generation_kernel_stats_{kvcache,skinny}.md)
 *   key 12: family 3 on four waves of 128x128 outputs (csrc/gemm8q.hip; env VALOR_GEMM_WAVE128): the 256x256 tile with one wave per SIMD and
 *          256 accumulator registers per lane -- 128 KiB instead of 192 KiB of LDS fragment reads per K-tile, same accumulation order, results
 *          bit-identical to the eight-wave kernel. 0 = never, 1 = wherever family 3 runs and the kernel has the layout (k-slow A and B: the
 *          weight gradients), 1000 (default) = measured per-class choice: the weight gradients with more than 48 K-tiles per workgroup
 *          (ViT and cross-K|V wgrads: 1.13-1.27 x alone, -1.9 ms per step, profiles/wave128_gemm_ab.json, profiles/wave128_gemm_by_grid_after.txt).
 *          A process default only: valor_gemm_policy has no field for it. */
int valor_gemm_set_policy(int key, int value);
/* 1 if valor_gemm would run this family-3 problem on csrc/gemm8q.hip under the policy in force (valor_gemm_kernel_for keeps answering 3) */
int valor_gemm_wave128_for(int dtype, int transA, int transB, int M, int N, int K, int heavy_epilogue);
/* K-loop schedule of the family-3 (256x256) kernel: 0 = eight barriers per K-tile, wave rows staggered by one barrier; 1 = software-pipelined:
 * two barriers per K-tile, fragment reads and LDS-DMA pieces between the MFMAs of the half-phase before their consumer. Same results (same
 * accumulation order). 1000 (default) = per problem: pipelined for forward / dgrad problems with K >= 2048 and for wgrads with at most 48 K-tiles
 * per workgroup. Returns the previous value; anything else only queries. Tuning / A-B hook (env VALOR_GEMM_8PH_SCHED). */
int valor_gemm_set_8ph_sched(int v);
/* schedule of the family-4 kernel: 0 = LOAD / MATH segments, one barrier per phase (the partner wave of every SIMD belongs to the CU's other
 * workgroup), 1 (default) = software-pipelined, two barriers per K-tile. Same results. Returns the previous value; anything but 0 / 1 only
 * queries. Tuning / A-B hook (env VALOR_GEMM_N8_SCHED). */
int valor_gemm_set_narrow_sched(int v);
/* workgroups of the family-4 kernel the runtime admits per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor at its 80 KiB of LDS): the
 * design point is 2; -1 on a runtime error. Needs a device. */
int valor_gemm_narrow_occupancy(void);
/* the same for the 512-thread workgroups of csrc/gemm8w.hip (policy key 10: family 4's NN problems on eight waves of 64x64 outputs): the
 * design point is 2 workgroups = four waves per SIMD (<= 128 registers per lane); -1 on a runtime error. Needs a device. */
int valor_gemm_wide_occupancy(void);

/* ---- cross-attention backward of EVERY decoder pass of a layer in one launch (csrc/attention_xu.hip). Replaces the autograd backward of
 * BertCrossAttention (model/bert.py:314-340) for the passes of model/pretrain.py:403-541 that share one projected K|V per layer (the
 * caption pass with its tva / tv / ta groups and the mlm pass, bert.py:448-457): K and V are read once and dK|dV WRITTEN once, where one
 * valor_attn_bwd per pass read K, V per pass and read-modified-wrote dK|dV from the second pass on.
 *   segs: HOST array of nseg (1 or 2) segment descriptors. Per segment q / o / dout / dq are [B, Sq, H*64] views (batch stride *_bs, row
 *   stride *_rs, elements), lse fp32 [B, H, Sq], kv_range int32 [B][2] = (first key, keys) or NULL, B = groups x kv_bmod: row r attends to
 *   K/V batch r % kv_bmod; (seed, offset) = the dropout window valor_attn_fwd used for that pass.
 *   k, v, dk, dv: [kv_bmod, Skv, H*64] views. dK|dV is overwritten (not accumulated). bf16 only, head_dim 64, Skv >= 64, at most ten 16-row
 *   query sub-tiles (sum over segments of B / kv_bmod x ceil(Sq / 16)); VALOR_ERR_ARG otherwise (callers fall back to valor_attn_bwd per
 *   pass; env VALOR_ATTN_XFUSED=0 forces that). */
typedef struct valor_xattn_seg {
    const void* q; const void* o; const void* dout; void* dq; const float* lse; const int* kv_range;
    int64_t q_bs, q_rs, o_bs, o_rs, do_bs, do_rs, dq_bs, dq_rs;
    int B, Sq;
    uint64_t seed, offset;
} valor_xattn_seg;
/* forward of the same passes in one launch (BertCrossAttention forward, bert.py:314-340): reads q, kv_range, (seed, offset) of every segment,
 * writes o ([B, Sq, H*64] view, strides o_bs / o_rs) and lse; dout / dq of the descriptors are ignored. Same domain and fallback rule
 * (valor_attn_fwd per pass) as the backward; the dropout keep pattern is the one valor_attn_fwd draws for (seed, offset). */
int valor_cross_attn_fwd_fused(void* stream, int dtype, const valor_xattn_seg* segs, int nseg, const void* k, const void* v, int H, int Skv,
                               int kv_bmod, int64_t k_bs, int64_t k_rs, int64_t v_bs, int64_t v_rs, float scale, float p_drop,
                               const uint64_t* rng_base);
int valor_cross_attn_bwd_fused(void* stream, int dtype, const valor_xattn_seg* segs, int nseg, const void* k, const void* v, void* dk, void* dv,
                               int H, int Skv, int kv_bmod, int64_t k_bs, int64_t k_rs, int64_t v_bs, int64_t v_rs, int64_t dk_bs,
                               int64_t dk_rs, int64_t dv_bs, int64_t dv_rs, float scale, float p_drop, const uint64_t* rng_base);

/* ---- fused bias + dropout + residual + LayerNorm.  Replaces apex FusedLayerNorm (apex/csrc/layer_norm_cuda_kernel.cu
 * :279-322 forward, :403-634 backward; wrapper apex/apex/normalization/fused_layer_norm.py:14-37) plus the elementwise ops
 * around it: bert.py:351-355,365-371,416-420 (post-LN), transformer.py:74-85 (pre-LN AST), clip.py:194-197 (pre-LN CLIP).
 *   z = dropout(x + bias)/(1-p) + residual ; y = LN(z; gamma, beta, eps).  z may alias x; any of bias/residual/gamma/beta/
 *   z/y may be NULL. mean/rstd: fp32 [rows].
 *   row_scale (may be NULL): fp32 [rows / rows_per_scale], (x + bias) is multiplied by row_scale[row / rows_per_scale] before the
 *   residual add -- VideoSwin's per-sample stochastic depth, drop_path (videoswin.py:40-49, 243-244), with
 *   row_scale = floor(keep + U[0,1)) / keep drawn by the caller. backward: dx = dz * row_scale (dx must not alias dres). */
int valor_ln_part_blocks(void);
/* kernel family of the fused LayerNorm: 1 (default) = half a wave per row with 16-byte accesses for bf16 rows of 256 / 512 / 768 /
 * 1024 columns in the forward (and in the backward at 1024 columns, where it measured faster), 2 = in forward and backward
 * everywhere, 0 = one wave per row everywhere. Same results (same arithmetic order per row up to the reduction tree, same
 * dropout windows). Returns the previous value, v < 0 only queries. Tuning / A-B hook. */
int valor_ln_set_variant(int v);
/* non-temporal accesses of the streaming LayerNorm kernels (bit mask; A/B hook, default 0, env VALOR_LN_NT): forward bit 0 = x loads,
 * 1 = y stores, 2 = z stores; backward bit 3 = dy / z / dz_in loads, 4 = dx / dres stores. Schedule hooks in the same mask: bit 5 = the
 * backward requests dz_in together with z / dy (measured -1 .. -3 %, within noise: off); bit 6 / bit 7 = force / forbid the loads-first
 * forward for bf16 rows of 768 columns (default: on from 65 536 rows, profiles/r04_ln_fwd_ab.txt). Returns the previous value, v < 0 only queries. */
int valor_ln_set_nt(int v);
int valor_bdrln_fwd(void* stream, int dtype, const void* x, const void* bias, const void* residual, const void* gamma,
                    const void* beta, void* z, void* y, float* mean, float* rstd, int64_t rows, int cols, float eps,
                    float p_drop, uint64_t seed, uint64_t offset, const float* row_scale, int64_t rows_per_scale,
                    const uint64_t* rng_base);
/* backward: dz = LN'(dy) + dz_in -> dres ; dx = dz * dropmask/(1-p). part_*: fp32 [valor_ln_part_blocks() * cols]
 * per-workgroup column partials of dgamma / dbeta / dbias (finish with valor_colsum_finalize). */
int valor_bdrln_bwd(void* stream, int dtype, const void* dy, const void* dz_in, const void* z, const float* mean,
                    const float* rstd, const void* gamma, void* dx, void* dres, float* part_dgamma, float* part_dbeta,
                    float* part_dbias, int64_t rows, int cols, float p_drop, uint64_t seed, uint64_t offset, const float* row_scale,
                    int64_t rows_per_scale, const uint64_t* rng_base);
int valor_colsum_finalize(void* stream, int dtype, const float* part, int nparts, int cols, void* out, int out_f32,
                          int accumulate);
/* up to three finalizations in ONE launch (NULL part = skip): dgamma / dbeta / dbias of valor_bdrln_bwd */
int valor_colsum_finalize3(void* stream, int dtype, const float* part0, void* out0, int acc0, const float* part1, void* out1,
                           int acc1, const float* part2, void* out2, int acc2, int nparts, int cols);
/* out[cols] (+)= column sums of x[rows, cols] (ld): nn.Linear bias gradients. part: fp32 [valor_ln_part_blocks()*cols]. */
int valor_colsum(void* stream, int dtype, const void* x, int64_t rows, int cols, int64_t ld, float* part, void* out,
                 int out_f32, int accumulate);

/* attention kernel selection (tuning / A-B hook): bit 0 = LDS-resident short-sequence self-attention kernels for
 * bf16 (S = Sq = Skv <= 256, no kv_range); bit 1 = key-stationary cross-attention kernels (few query rows, many keys,
 * grouped kv_range); bit 2 = one wave per (sequence, head) for <= 4 query rows against <= 256 keys without dropout / kv_range, fp32
 * and bf16 (the decoding step against a K|V cache); 0 = streaming kernels only. Default 7. Returns the previous value; v < 0 queries. */
int valor_attn_set_variant(int v);
/* One decoding step of caption generation against per-sequence self-attention K|V slots (the reference re-runs every text row at every
 * step: pretrain.py:988-1188 over bert.py:272-288): Sq <= 4 new rows per sequence, Skv <= 256 slots, additive fp32 mask, no dropout.
 * key_row (int32 [B][key_row_bs], device; may be null): slot j of sequence b is read from batch row key_row[b][j] of k / v -- the
 * sequences of a beam search read their ancestors' slots where they were written (`_adjust_tensor`, pretrain.py:1161-1180, moves
 * tensors instead). Strides as valor_attn_fwd. */
int valor_attn_decode_fwd(void* stream, int dtype, const void* q, const void* k, const void* v, void* o, float* lse,
                          int B, int H, int Sq, int Skv, int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs,
                          int64_t v_bs, int64_t v_rs, int64_t o_bs, int64_t o_rs, const float* mask, int64_t mask_bs,
                          int64_t mask_rs, const int* key_row, int64_t key_row_bs, float scale);
/* LDS-resident self-attention backward: 1 (default, env VALOR_ATTN_PIPE) = persistent workgroups (one per CU) that walk (batch, head)
 * items with the K / V and Q / dO LDS images double-buffered across the dQ and the dK / dV phase, so the loads and stores of one item
 * overlap the arithmetic of its neighbours (used when batch x heads >= 2 x the CU count; sequences of <= 160 rows run mode 2 instead);
 * 0 = one workgroup of 8 waves x 32-row blocks per (batch, head); 2 = one workgroup of 16 waves x 16-row blocks per (batch, head) (four
 * waves per SIMD); 3 = mode 1 with the FIRST version of the persistent kernel (round 6 added a second: phase operands out of LDS / prefetched
 * under the dK / dV loop, 16-byte stores -- bit-identical to the first, used when the gradient rows are 16-byte aligned and there is no
 * additive mask). Modes 0 and 2 are bit-identical, modes 1 / 3 differ from them in the summation order of delta only. Returns the previous
 * value, v < 0 only queries. */
int valor_attn_set_res_pipeline(int v);

/* ---- flash attention, head_dim 64.  Replaces BertSelfAttention (bert.py:272-288), BertCrossAttention (bert.py:314-340,
 * K/V = [video|audio] tokens, grouping bert.py:448-455), AST MultiHeadAttention (transformer.py:115-130) and CLIP's
 * nn.MultiheadAttention (clip.py:186-192, mask clip.py:407-414).  Element (b,row,h,d) of q/k/v/o lives at
 * base + b*bs + row*rs + h*64 + d.  mask: additive fp32 [*, Sq, >=len] indexed (b*mask_bs + q*mask_rs + local key).
 * kv_range: int32 [B][2] (start,len) rows of the K/V buffer batch b attends to; kv_bmod>0: K/V batch = b % kv_bmod
 * (modality-grouped cross-attention with ONE shared K/V projection). lse: fp32 [B,H,Sq]. */
int valor_attn_fwd(void* stream, int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B,
                   int H, int Sq, int Skv, int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs,
                   int64_t v_rs, int64_t o_bs, int64_t o_rs, const float* mask, int64_t mask_bs, int64_t mask_rs,
                   const int* kv_range, int kv_bmod, float scale, float p_drop, uint64_t seed, uint64_t offset,
                   const uint64_t* rng_base);
/* accumulate_dkdv != 0: dk/dv += (several query passes share one K/V set; gradients meet in one buffer) */
int valor_attn_bwd(void* stream, int dtype, const void* q, const void* k, const void* v, const void* o, const float* lse,
                   const void* dout, void* dq, void* dk, void* dv, float* delta, int B, int H, int Sq, int Skv,
                   int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs, int64_t v_rs, int64_t o_bs,
                   int64_t o_rs, int64_t do_bs, int64_t do_rs, int64_t dq_bs, int64_t dq_rs, int64_t dk_bs, int64_t dk_rs,
                   int64_t dv_bs, int64_t dv_rs, const float* mask, int64_t mask_bs, int64_t mask_rs, const int* kv_range,
                   int kv_bmod, float scale, float p_drop, uint64_t seed, uint64_t offset, int accumulate_dkdv,
                   const uint64_t* rng_base);

/* ---- VideoSwin 3-D shifted-window attention, head_dim 32 (videoswin.py:137-163 with the roll / window_partition /
 * window_reverse around it :205-220, relative position bias :146-148, shift mask :150-154,272-285), in place on the fused QKV
 * GEMM output in natural token order. qkv [B*rows_per_sample][3C] (C = heads*32; q | k | v), o [B*rows_per_sample][C].
 * rowmap int32 [nW*N]: token row (inside a sample) of slot n of window w (roll + partition; outputs are scattered back through
 * it). rel int32 [N]: linearised (d,h,w) of a slot in the FULL window, bias(i,j) = table[rel[i]-rel[j]+relc][head]; table
 * [table_rows][heads]. label uint8 [nW*N] region ids of the shift mask (NULL = unshifted): -100 where labels differ.
 * lse fp32 [B*nW][heads][N]. bf16: N <= 448; fp32 (parity mode): forward N <= 448, backward N <= 192 (the window is LDS resident; VALOR_ERR_ARG beyond). */
/* kernel family bits for A/B tests (bf16): 1 = LDS-DMA dQ pass, 2 = LDS-DMA forward, 4 = LDS-DMA dK/dV pass (default 7); 8 = the first
 * version of the LDS-DMA dQ pass instead of the look-ahead version, 16 = four query partitions instead of two in it, 32 / 64 = the dK/dV
 * pass / the forward without their operand look-ahead (windows up to 256 slots); every combination computes the same bits. Returns the
 * previous value, v < 0 only queries */
int valor_win_attn_set_variant(int v);
int valor_win_attn_workspace_floats(int B, int nW, int N, int heads);   /* fp32 elements the backward needs */
int valor_win_attn_fwd(void* stream, int dtype, const void* qkv, void* o, float* lse, const int* rowmap, const int* rel,
                       const uint8_t* label, const void* table, int B, int nW, int N, int heads, int table_rows, int relc,
                       int rows_per_sample, float scale);
/* dqkv [rows][3C] (every row of every window is written); dtable [table_rows][heads] (+= if accumulate_dtable); delta fp32
 * like lse; rel_inv int32 [relc + 1]: slot whose rel is m (or -1); workspace: valor_win_attn_workspace_floats() fp32 (dense
 * per-window-group sums of dS, reduced and gathered into the table after the dQ pass) */
int valor_win_attn_bwd(void* stream, int dtype, const void* qkv, const void* o, const float* lse, const void* dout, void* dqkv,
                       float* delta, const int* rowmap, const int* rel, const int* rel_inv, const uint8_t* label, const void* table,
                       void* dtable, int accumulate_dtable, void* workspace, int64_t workspace_bytes, int B, int nW, int N, int heads,
                       int table_rows, int relc, int rows_per_sample, float scale);

/* ---- native gradient reducer over RCCL (csrc/reducer.hip): the bucketed gradient all-reduce of the data-parallel step. Replaces the
 * reducer of torch DDP (train_utils.py:232; model of the same structure: apex/apex/parallel/distributed.py:320-470). RCCL is bound with
 * dlopen at first use (the copy already loaded by torch.distributed if there is one, $VALOR_RCCL_LIB, the default search path);
 * VALOR_ERR_LAUNCH if it cannot be bound or a RCCL / HIP call fails. Nothing below synchronises the host.
 *   unique_id:      rank 0 fills 128 bytes (ncclGetUniqueId); the caller hands the same bytes to every rank (torch.distributed broadcast).
 *   create:         one communicator (ncclCommInitRank: collective over all `world` ranks), one communication stream, one event per bucket.
 *                   Bucket i = elements [offsets[i], offsets[i] + counts[i]) of the flat gradient arena at grad_base (dtype bf16 / fp32),
 *                   summed in place. mode 0 = all-reduce, 1 = reduce-scatter + all-gather on the in-place shards (counts[i] % world == 0,
 *                   else that bucket falls back to all-reduce).
 *   launch_bucket:  the communication stream waits for the current tail of every stream in compute_streams (all that may still be writing
 *                   gradients of this bucket) and enqueues the collective.
 *   wait:           `stream` waits for every bucket launched since the previous wait.
 *   destroy:        drains the communication stream, frees the communicator, events and stream (NULL is a no-op). */
int valor_reducer_unique_id(void* id128);
int valor_reducer_create(void** out, const void* id128, int rank, int world, int dtype, void* grad_base, const int64_t* offsets,
                         const int64_t* counts, int nbuckets, int mode);
int valor_reducer_launch_bucket(void* reducer, int bucket, void* const* compute_streams, int nstreams);
int valor_reducer_wait(void* reducer, void* stream);
int valor_reducer_destroy(void* reducer);

/* ---- softmax cross-entropy over the vocabulary: F.cross_entropy on the masked rows (pretrain.py:444,457,469,498).
 * logits [rows, V] with leading dim ld; backward overwrites the logits (and zero-fills the ld padding) with
 * (softmax - onehot) * (*gscale_dev) * gmul.
 * A label outside [0, V) marks an ignored row: loss_rows = 0, lse is still written, and every backward entry point below writes exact
 * zeros over that row (padding included). The other rows are not renormalised by the number of valid rows: gmul is the caller's. */
int valor_xent_fwd(void* stream, int dtype, const void* logits, const int64_t* labels, float* loss_rows, float* lse,
                   int64_t rows, int V, int64_t ld);
int valor_xent_bwd(void* stream, int dtype, void* logits_inout, const int64_t* labels, const float* lse,
                   const float* gscale_dev, float gmul, int64_t rows, int V, int64_t ld);
/* the same with label smoothing (LabelSmoothing, model/pretrain.py:46-61,839-840): target 1 - smoothing on the label, smoothing / (V - 1)
 * elsewhere; row loss = KL(target || softmax), backward (softmax - target) * g. smoothing in [0, 1); 0 = valor_xent_fwd / _bwd. */
int valor_xent_smooth_fwd(void* stream, int dtype, const void* logits, const int64_t* labels, float* loss_rows, float* lse,
                          int64_t rows, int V, int64_t ld, float smoothing);
int valor_xent_smooth_bwd(void* stream, int dtype, void* logits_inout, const int64_t* labels, const float* lse,
                          const float* gscale_dev, float gmul, int64_t rows, int V, int64_t ld, float smoothing);
int valor_mean_f32(void* stream, const float* x, int64_t n, float* out);
/* the reward-weighted caption loss of SCST (reward_loss, pretrain.py:166-173: the mean over labelled positions of -r_i logP):
 * valor_xent_weighted_bwd = valor_xent_bwd with g_i = (*gscale_dev) * gmul * w_rows[i] (w_rows fp32 [rows]; null: valor_xent_bwd);
 * valor_weighted_mean_f32: *out = sum_i w[i] * x[i] / n. Neither reads anything back to the host. */
int valor_xent_weighted_bwd(void* stream, int dtype, void* logits_inout, const int64_t* labels, const float* lse, const float* w_rows,
                            const float* gscale_dev, float gmul, int64_t rows, int V, int64_t ld);
int valor_weighted_mean_f32(void* stream, const float* x, const float* w, int64_t n, float* out);

/* ---- MGA fine-grained contrastive: compute_fine_matrix_slice (pretrain.py:191-211) + contrastive_loss
 * (modeling.py:418-433). S = featA . featB^T comes from valor_gemm (fp32 [B*T, ldS]). */
int valor_fine_weight_softmax(void* stream, const float* raw, const float* mask, float* w, int rows, int n);
int valor_fine_weight_softmax_bwd(void* stream, const float* w, const float* dw, float* draw, int rows, int n);
int valor_fine_reduce_fwd(void* stream, const float* S, int64_t ldS, const float* maskA, const float* maskB,
                          const float* wA, const float* wB, float* score, float* A2B, float* B2A, uint8_t* idxA,
                          uint8_t* idxB, int B, int T, int Nv);
/* evaluation: the score matrix alone for NA text items x NB video / audio items (rectangular, nothing saved for a backward):
 * test.py:534-660 -> VALOR.compute_fine_matrix (pretrain.py:178-211). S fp32 [NA*T, ldS]; maskA, wA [NA,T]; maskB, wB [NB,Nv];
 * score [NA,NB]; NA <= 65535 per call (the reference itself slices NA by 100 above 1200 items, pretrain.py:179-186). */
int valor_fine_scores(void* stream, const float* S, int64_t ldS, const float* maskA, const float* maskB, const float* wA,
                      const float* wB, float* score, int NA, int NB, int T, int Nv);
int valor_infonce_fwd(void* stream, const float* score, const float* k_dev, float* lse_r, float* lse_c, float* loss, int B);
int valor_infonce_bwd(void* stream, const float* score, const float* k_dev, const float* lse_r, const float* lse_c,
                      const float* g_dev, float* dscore, float* dk, float* part, int B);
int valor_fine_reduce_bwd(void* stream, int dtype, const float* dscore, const float* maskA, const float* maskB,
                          const float* wA, const float* wB, const float* A2B, const float* B2A, const uint8_t* idxA,
                          const uint8_t* idxB, void* dS, int64_t ldS, float* dwA, float* dwB, int B, int T, int Nv);
/* FUSED fine-grained contrastive (pretrain.py:191-211 without any [A*T, B*Nv] tensor): bf16 features featA [NA, T, D], featB
 * [NB, Nv, D] (D % 64 == 0; T, Nv <= 64) -> score [NA, NB] and, unless all four are null (evaluation), A2B [NA, NB, T] / B2A
 * [NA, NB, Nv] (the directional maxima, fp32) and their first-arg-max bytes idxA / idxB -- the outputs of valor_fine_reduce_fwd, with
 * the token x token dot products accumulated on the matrix pipe and reduced in registers. Backward: valor_fine_weight_grad for the
 * token weights; valor_fine_ds_chunk writes d(sims) of the texts [a0, a0 + na) as a dense [na * T, ldS] tile (column b * Nv + v) from
 * the argmax bytes, which two valor_gemm calls per chunk contract with the features. valor_fine_set_fused: 1 (default, env
 * VALOR_FINE_FUSED) / 0 = what the host wrapper uses; < 0 queries. */
int valor_fine_fused_fwd(void* stream, const void* featA, const void* featB, const float* maskA, const float* maskB, const float* wA,
                         const float* wB, float* score, float* A2B, float* B2A, uint8_t* idxA, uint8_t* idxB, int NA, int NB, int T,
                         int Nv, int D);
int valor_fine_ds_chunk(void* stream, int dtype, const float* dscore, const float* maskA, const float* maskB, const float* wA,
                        const float* wB, const uint8_t* idxA, const uint8_t* idxB, void* dS, int64_t ldS, int a0, int na, int NB, int T,
                        int Nv);
int valor_fine_weight_grad(void* stream, const float* dscore, const float* A2B, const float* B2A, float* dwA, float* dwB, int B, int T,
                           int Nv);
int valor_fine_set_fused(int v);

/* ---- retrieval evaluation: the rank of every ground truth in a score matrix, without a sort (csrc/retrieval.hip). Replaces
 * compute_dualsoftmax_forward / _backward and the sort + tolist + list.index of compute_metric_ret (test.py:685-775).
 *   score fp32 [Nt, ld] (ld >= Nv): rows = texts (the A side), columns = clips (the B side). gt_col int32 [Nt]: the column of each
 *   text's clip. col_ptr int32 [Nv + 1], col_rows int32 [nnz]: the texts of every clip as a CSR list (col_rows[col_ptr[j] ..
 *   col_ptr[j + 1]) = the rows i whose clip is column j; nnz = Nt unless two columns carry the same clip id and share their texts,
 *   test.py:746-748); read only when rank_b is given, entries outside [0, nnz) / [0, Nt) are skipped.
 *   dual != 0 (the reference's dual_softmax): lse_col[j] = logsumexp_i(score[i,j] * inv_temp) and lse_row[i] = logsumexp_j(...) are
 *   computed (and WRITTEN to lse_col fp32 [Nv] / lse_row fp32 [Nt], natural log, where the pointer is not NULL) and
 *     x[i,j] = score[i,j] * exp(score[i,j] * inv_temp - lse_col[j]) * Nt     (test.py:694, softmax over dim 0 times len(score))
 *     y[i,j] = score[i,j] * exp(score[i,j] * inv_temp - lse_row[i]) * Nv     (test.py:710)
 *   otherwise x = y = score and inv_temp / lse_* are ignored.
 *   rank_f int32 [Nt]: rank_f[i] = #{j : x[i,j] > x[i,g]} + #{j < g : x[i,j] == x[i,g]}, g = gt_col[i]; -1 if g is outside [0, Nv).
 *   rank_b int32 [Nv] (NULL = forward only): with m_j = max{y[i,j] : gt_col[i] == j} and i* the lowest such i that reaches it,
 *   rank_b[j] = #{i : y[i,j] > m_j} + #{i < i* : y[i,j] == m_j} = the minimum over the clip's texts of their position in the column
 *   (test.py:743-750); -1 for a clip without a text.
 *   TIE RULE: equal values rank in index order, i.e. the position in a STABLE descending sort. torch.sort(descending=True) without
 *   stable=True, which the reference calls, leaves the order of equal values undefined; this is the one deterministic choice.
 *   A NaN compares as not greater (a NaN ground truth therefore gets rank 0): no rank leaves [0, Nv) / [0, Nt).
 *   workspace: valor_retrieval_workspace_bytes() bytes, 16-byte aligned (column partials of the reductions; no [Nt, Nv] temporary, no
 *   float atomics). Passes over the matrix: 1 without dual, 2 with it. 16-byte loads when ld % 4 == 0 and score is 16-byte aligned.
 *   Nt == 0 or Nv == 0: no-op. VALOR_ERR_ARG on a null / misaligned pointer, ld < Nv, a short workspace, dual with inv_temp <= 0. */
int valor_retrieval_workspace_bytes(int Nt, int Nv, int64_t* bytes);
int valor_retrieval_ranks(void* stream, const float* score, int64_t ld, const int* gt_col, const int* col_ptr, const int* col_rows,
                          int nnz, float inv_temp, int dual, float* lse_row, float* lse_col, int* rank_f, int* rank_b, void* workspace,
                          int64_t workspace_bytes, int Nt, int Nv);

/* ---- retrieval search: the k best columns of every row of a score matrix, streaming over column chunks (csrc/search.hip; the
 * selection under valor_amd/search.py RetrievalIndex).
 *   score fp32 [R, ld] (ld >= C). The candidates of row r are the pairs (score[r, c], col_base + c), c < C, and, with merge != 0, the
 *   entries already in top_val[r, :] / top_idx[r, :] whose index is >= 0. top_val fp32 [R, k] and top_idx int64 [R, k] receive the k
 *   best candidates, best first, under ONE total order: value descending, then index ascending. A NaN ranks below every number, -inf
 *   included (NaNs among themselves by index): the opposite of torch.topk, and the rule of valor_retrieval_ranks, where a NaN compares
 *   as not greater. -0 equals +0. With fewer than k candidates the remaining slots hold -inf / -1: every index written is a
 *   candidate's or -1, never a sentinel a later gather could dereference.
 *   The result does not depend on how the work is split (integer keys, no float atomics), so folding the chunks of a bank one by one
 *   (merge = 1, col_base = the chunk's first clip) equals one pass over the whole row. 1 <= k <= 256; 0 <= col_base and col_base + C
 *   < 2^63 - 1 (indices beyond 2^31 are fine). 16-byte loads when ld % 4 == 0 and score is 16-byte aligned, 4-byte loads otherwise.
 *   workspace: valor_topk_workspace_bytes(R, C, k) bytes, 16-byte aligned, caller-owned (the k best keys of every column segment of
 *   every row; at most one segment per 4096 columns, each a multiple of 1024 columns). Two launches: rows x segments workgroups, then one workgroup per row.
 *   R == 0: no-op. VALOR_ERR_ARG before anything is launched on a null / misaligned pointer, ld < C, k outside [1, 256], a negative or
 *   overflowing col_base, a short or misaligned workspace. */
int valor_topk_workspace_bytes(int R, int C, int k, int64_t* bytes);
int valor_topk_rows(void* stream, const float* score, int64_t ld, int R, int C, int64_t col_base, int k, int merge, float* top_val,
                    int64_t* top_idx, void* workspace, int64_t workspace_bytes);

/* ---- retrieval search: the selection with a column filter and one result per group (csrc/search_select.hip; RetrievalIndex after
 * remove(), and search(where=, collapse=)). A superset of valor_topk_rows: score, ld, R, C, col_base, k, merge, top_val, top_idx, the
 * total order (value descending, then index ascending, a NaN below every number, -0 == +0), the -inf / -1 padding, the streaming
 * contract and the independence of the result from how the work is split are that entry's. The index of a candidate is
 * i = col_base + c for a column, top_idx[r, p] for an entry merged in; both additions are addressed by it.
 *   keep   uint8 (a bool array as it is), or NULL: every candidate is eligible. The candidate i of row r is eligible iff
 *          keep[r * keep_ld + i] != 0; keep_ld == 0: one array shared by all rows. With merge, the entries already in top_idx are
 *          checked too: one that is no longer eligible drops out.
 *   group  int32, 4-byte aligned, or NULL: no grouping. g = group[r * group_ld + i] (group_ld == 0: shared). The eligible candidates of
 *          one id g >= 0 are ONE result, represented by the best of them under the total order (equal values: the lowest index); a
 *          candidate with g < 0 is a group of its own. top_val / top_idx receive the k best representatives, best first: no group id
 *          appears twice in a row. A later, better member (a later column, segment or merged chunk) replaces its group's
 *          representative, a later, worse one vanishes; with fewer than k eligible groups the remaining slots hold -inf / -1.
 *   Both arrays must cover every index the call meets: col_base + C entries, and with merge every index >= 0 in top_idx. The keep
 *   byte and the group id are read only for candidates that beat the running threshold (the k-th best distinct representative;
 *   none while fewer than k groups are known), so the pruning stays exact. With keep and group NULL the outputs equal
 *   valor_topk_rows' bit for bit.
 *   workspace: valor_topk_select_workspace_bytes(R, C, k) bytes, 16-byte aligned (the layout of valor_topk_workspace_bytes: the group of
 *   a segment's key is read through `group` again by the merge). Two launches, as valor_topk_rows.
 *   R == 0: no-op. VALOR_ERR_ARG before anything is launched on every ground valor_topk_rows names, a negative keep_ld or group_ld,
 *   a misaligned group. */
int valor_topk_select_workspace_bytes(int R, int C, int k, int64_t* bytes);
int valor_topk_rows_select(void* stream, const float* score, int64_t ld, int R, int C, int64_t col_base, int k, int merge,
                           const uint8_t* keep, int64_t keep_ld, const int32_t* group, int64_t group_ld, float* top_val, int64_t* top_idx,
                           void* workspace, int64_t workspace_bytes);

/* ---- retrieval search on an fp8 clip bank (csrc/search_fp8.hip; valor_amd/search.py RetrievalIndex with bank_dtype="fp8"). gfx950.
 * valor_fp8_quantize_rows: every row of x (dtype VALOR_DT_BF16 / VALOR_DT_F32, [rows, ld], ld >= cols, cols % 16 == 0, rows 16-byte
 *   aligned) becomes cols OCP e4m3fn codes (uint8 [rows, cols], dense, 16-byte aligned) and one fp32 scale. All in fp32,
 *   round-to-nearest: amax = max |x|; amax < 2^-64: scale 0, every code 0x00; else scale = amax / 448, inv = 448 / amax,
 *   code = e4m3fn(min(max(x * inv, -448), 448)), nearest-even, subnormals and sign kept. The caller keeps non-finite values out
 *   (search.py reduces isfinite over the incoming rows first). rows == 0: no-op. VALOR_ERR_ARG before any launch on a null or
 *   misaligned pointer, an unknown dtype, ld < cols, cols <= 0 or cols % 16 != 0.
 * valor_fine_fused_fwd_fp8: the scores-only mode of valor_fine_fused_fwd on such rows: score[a, b] fp32 [NA, NB] of
 *   compute_fine_matrix_slice (pretrain.py:191-211) on code * scale, i.e. sim[a,b,t,v] = scaleA[a,t] scaleB[b,v] sum_d codeA codeB.
 *   codesA uint8 [NA, T, D], scaleA fp32 [NA, T], codesB [NB, Nv, D], scaleB [NB, Nv]; masks and SOFTMAXED token weights as in
 *   valor_fine_fused_fwd. D % 128 == 0, 1 <= T, Nv <= 64, each code tensor below 0x7f000000 bytes and 16-byte aligned. No backward
 *   pass exists for it. NA == 0 or NB == 0: no-op. VALOR_ERR_ARG before any launch otherwise. */
int valor_fp8_quantize_rows(void* stream, int dtype, const void* x, int64_t ld, int64_t rows, int cols, uint8_t* codes, float* scales);
int valor_fine_fused_fwd_fp8(void* stream, const uint8_t* codesA, const float* scaleA, const uint8_t* codesB, const float* scaleB,
                             const float* maskA, const float* maskB, const float* wA, const float* wB, float* score, int NA, int NB,
                             int T, int Nv, int D);

/* ---- retrieval search on an MXFP4 clip bank (csrc/search_mx.hip; valor_amd/search.py RetrievalIndex with bank_dtype="mxfp4"). gfx950.
 * The OCP MX v1.0 block-scaled forms: one E8M0 scale byte (2^(byte - 127)) per block of 32 consecutive elements of a row. The format
 * ids are the hardware's own (the cbsz / blgp field of v_mfma_scale_f32_16x16x128_f8f6f4).
 * valor_mx_quantize_rows: every row of x (dtype VALOR_DT_BF16 / VALOR_DT_F32, [rows, ld], ld >= cols, cols % 32 == 0, rows 16-byte
 *   aligned) becomes codes (fmt VALOR_MX_E4M3: uint8 [rows, cols]; VALOR_MX_E2M1: uint8 [rows, cols / 2], element 2i in the low nibble
 *   of byte i; dense, 16-byte aligned) and scale bytes uint8 [rows, cols / 32]. Per block: amax = max |x|, e = floor(log2 amax) (a zero
 *   or fp32-subnormal amax counts as -127), s = max(e - emax, -127) with emax 8 (e4m3) / 2 (e2m1), scale byte s + 127 (never 255),
 *   code = RNE(min(max(x * 2^-s, -max), max)) with max 448 / 6: the power-of-two multiply is exact, ties go to the even code, the
 *   sign of zero and the element format's subnormals are kept; an all-zero block has byte 0 and zero codes. The caller keeps
 *   non-finite values out. rows == 0: no-op. VALOR_ERR_ARG before any launch on a null or misaligned pointer, an unknown dtype or fmt,
 *   ld < cols, cols <= 0 or cols % 32 != 0.
 * valor_fine_fused_fwd_mx: the scores-only mode of valor_fine_fused_fwd on such rows: score[a, b] fp32 [NA, NB] of
 *   compute_fine_matrix_slice (pretrain.py:191-211) on the dequantised rows code * 2^(byte - 127). codesA uint8 [NA, T, D] (MX e4m3,
 *   the queries), scaleA uint8 [NA, T, D / 32]; codesB uint8 [NB, Nv, D / 2] (MX e2m1, the bank), scaleB uint8 [NB, Nv, D / 32]; masks
 *   and SOFTMAXED token weights as in valor_fine_fused_fwd. The element products and the scales are exact in fp32; only the
 *   accumulation rounds. D % 128 == 0, 1 <= T, Nv <= 64, each code tensor below 0x7f000000 bytes and 16-byte aligned, the scale
 *   tensors 4-byte aligned. No backward pass exists for it. NA == 0 or NB == 0: no-op. VALOR_ERR_ARG before any launch otherwise. */
#define VALOR_MX_E4M3 0
#define VALOR_MX_E2M1 4
int valor_mx_quantize_rows(void* stream, int dtype, const void* x, int64_t ld, int64_t rows, int cols, int fmt, uint8_t* codes,
                           uint8_t* scales);
int valor_fine_fused_fwd_mx(void* stream, const uint8_t* codesA, const uint8_t* scaleA, const uint8_t* codesB, const uint8_t* scaleB,
                            const float* maskA, const float* maskB, const float* wA, const float* wB, float* score, int NA, int NB,
                            int T, int Nv, int D);

/* ---- retrieval search, pair scores: every query against ITS OWN candidate list, read by index from a feature store (csrc/search_pairs.hip;
 * valor_amd/search.py score_pairs, RetrievalIndex.rescore / search(within=) / the two-stage search of an fp8 bank). gfx950.
 *   featA bf16 [NA, T, D]; maskA (the text mask) and wA (the SOFTMAXED text token weights) fp32 [NA, T], as in valor_fine_fused_fwd.
 *   storeB bf16 [NS, Nv, D]: any device-addressable feature store (a bank, or a staging buffer of gathered rows; it may exceed 2 GiB);
 *   wStoreB fp32 [NS, Nv]: its SOFTMAXED clip token weights. The clip mask is all ones and implicit. cand int64 [NA, ld_cand], of
 *   which C columns are read. score fp32 [NA, ld_score]: score[a, c], c < C, is the scores-only result of valor_fine_fused_fwd
 *   (compute_fine_matrix_slice, pretrain.py:191-211) for the pair (query a, clip cand[a, c]), with that kernel's padding law and
 *   reduction order; columns c >= C are not written. A candidate outside [0, NS), -1 included, is never dereferenced: its score is
 *   -inf. Duplicates are scored like any other candidate. D % 64 == 0 (D <= 2^20), 1 <= T, Nv <= 64; featA and storeB 16-byte
 *   aligned, cand 8-byte aligned. One launch; no workspace. NA == 0 or C == 0: no-op. VALOR_ERR_ARG before any launch on a null or
 *   misaligned pointer, ld_cand < C, ld_score < C, a negative count or a shape outside the coverage. */
int valor_fine_score_pairs(void* stream, const void* featA, const float* maskA, const float* wA, const void* storeB,
                           const float* wStoreB, int64_t NS, const int64_t* cand, int64_t ld_cand, float* score, int64_t ld_score,
                           int NA, int C, int T, int Nv, int D);

/* ---- retrieval search, pair alignments: the token-level detail of the same pairs (csrc/search_align.hip; valor_amd/search.py align_pairs,
 * RetrievalIndex.explain / search(explain=True)). gfx950. Inputs, coverage and alignment as valor_fine_score_pairs. For the pair
 * (query a, clip b = cand[a, c]), with valor_fine_fused_fwd's padding law and tie rule:
 *     x[t,v] = S[t,v] * maskA[a,t]                  (the clip mask is all ones and implicit)
 *     a2b[t] = max_v x, idx_a[t] = the FIRST arg max;   b2a[v] = max_t x, idx_b[v] = the FIRST arg max
 *     termA[t] = 0.5 * (wA[t] * a2b[t]);   termB[v] = wB[v] != 0 ? 0.5 * (wB[v] * b2a[v]) : 0
 *     credit_b[v] = termB[v], then + termA[t] for every t in ascending order with idx_a[t] == v
 *     credit_a[t] = termA[t], then + termB[v] for every v in ascending order with idx_b[v] == t
 *   every step of the credits in fp32, rounded on its own (no fma), so a host loop in fp32 reproduces them bit for bit from the
 *   kernel's maxima and indices; in exact arithmetic either credit array sums to the pair's score.
 *   Outputs are dense, C columns per query, and each may be NULL on its own, except that an index array comes with its value array:
 *   score fp32 [NA, C] (valor_fine_score_pairs' expression); a2b fp32 + idx_a uint8 [NA, C, T]; b2a fp32 + idx_b uint8 [NA, C, Nv];
 *   credit_a fp32 [NA, C, T]; credit_b fp32 [NA, C, Nv]; sim fp32 [NA, C, T, Nv] = x itself (64-bit offsets).
 *   A candidate outside [0, NS), -1 included, is never dereferenced: its score is -inf, its index bytes 255, its other floats 0.
 *   One launch, no workspace, no float atomics: the same input gives the same bits. NA == 0 or C == 0: no-op. VALOR_ERR_ARG before any
 *   launch on a null input pointer, a misaligned pointer, ld_cand < C, a negative count, a shape outside the coverage, or an index
 *   array without its value array or the other way round. */
int valor_fine_align_pairs(void* stream, const void* featA, const float* maskA, const float* wA, const void* storeB,
                           const float* wStoreB, int64_t NS, const int64_t* cand, int64_t ld_cand, int NA, int C, int T, int Nv, int D,
                           float* score, float* a2b, uint8_t* idx_a, float* b2a, uint8_t* idx_b, float* credit_a, float* credit_b,
                           float* sim);

/* ---- fused multi-tensor AdamW + global-norm clip over flat arenas.  Replaces optim/adamw.py:40-103, optim/misc.py:66-77
 * (10 param groups), torch clip_grad_norm_ (train_utils.py:358-360) and apex-amp's master<->model copies
 * (apex/apex/amp/_process_optimizer.py:14-22). n % valor_adamw_chunk() == 0; chunk_group: int8 [n/chunk], -1 = skip. */
int valor_adamw_chunk(void);
/* non-temporal state accesses of valor_adamw (bit 0 loads, bit 1 stores; A/B hook, env VALOR_ADAMW_NT); returns the previous value, v < 0 queries */
int valor_adamw_set_nt(int v);
int valor_adamw(void* stream, int dtype, float* master, float* exp_avg, float* exp_avg_sq, void* grad, void* param,
                const int8_t* chunk_group, int64_t n, const float* lr, const float* wd, int ngroups, float beta1,
                float beta2, float eps, int step, int correct_bias, const float* gscale_dev, int zero_grad);
/* valor_adamw with the Adam step count on the device: tensor_step int32 [ntensors] (the count of each tensor before this step),
 * chunk_tensor int32 [n/chunk] (tensor of each chunk; a tensor's chunks are consecutive), chunk_bc fp32 scratch [2*n/chunk]. The
 * bias correction of every chunk uses its tensor's count + 1; afterwards the count of every active tensor advances by one, unless
 * the step was skipped (non-finite *gscale_dev). Three launches, no host sync. */
int valor_adamw_counted(void* stream, int dtype, float* master, float* exp_avg, float* exp_avg_sq, void* grad, void* param,
                        const int8_t* chunk_group, const int32_t* chunk_tensor, int32_t* tensor_step, int ntensors, float* chunk_bc,
                        int64_t n, const float* lr, const float* wd, int ngroups, float beta1, float beta2, float eps,
                        int correct_bias, const float* gscale_dev, int zero_grad);
/* total_norm = sqrt(sum of squares of the active chunks) * norm_mul; gscale = norm_mul * min(1, max_norm / (total_norm + 1e-6)),
 * max_norm <= 0: no clipping; gscale = NaN if total_norm is not finite (valor_adamw* then skip the update and only clear the
 * gradients). partial: fp32 scratch >= 1024 floats. */
int valor_grad_norm_clip(void* stream, int dtype, const void* grad, const int8_t* chunk_group, int64_t n, float norm_mul,
                         float max_norm, float* partial, float* total_norm, float* gscale);

/* ---- data-movement kernels around the core */
/* conv(kernel=stride=P) as GEMM: clip.py:227,261 ; modeling.py:744,752 */
int valor_patchify(void* stream, int dtype, const float* in, void* out, int N, int C, int H, int W, int P, int64_t ld_out);
/* ld_out: row stride of `out` in elements (0 = C*P*P); > C*P*P when rows are padded to whole 16-byte GEMM chunks (ViT-L/14:
 * 588 -> 592; the pad columns are the caller's to zero). P must be even. */
/* VideoSwin PatchEmbed3D (videoswin.py:361-369): Conv3d(kernel (2,P,P), stride (1,P,P)) over the clip with one zero frame
 * appended, as a GEMM operand. in: fp32 [B, F, C, H, W] (the batch layout of data/data.py:423-428, no transpose);
 * out [B*F*(H/P)*(W/P)][C*2*P*P], column (c*2 + kd)*P*P + i*P + j = in[b][d + kd][c][py*P + i][px*P + j] (0 for d + kd == F) */
int valor_patchify3d(void* stream, int dtype, const float* in, void* out, int B, int F, int C, int H, int W, int P);
/* mean over groups of X consecutive rows (VideoSwin pooling, modeling.py:388-389): out[g] = mean_x in[g*X + x]; backward
 * din[g*X + x] = dout[g] / X */
int valor_group_mean_fwd(void* stream, int dtype, const void* in, void* out, int64_t groups, int X, int E);
int valor_group_mean_bwd(void* stream, int dtype, const void* dout, void* din, int64_t groups, int X, int E);
/* [cls ; patches (+bias)] + pos: clip.py:264-265 ; modeling.py:755-760 */
int valor_assemble_tokens_fwd(void* stream, int dtype, const void* patches, const void* cls, const void* pos,
                              const void* bias, void* out, int N, int Pn, int E);
int valor_assemble_tokens_bwd(void* stream, int dtype, const void* dout, void* dpatches, void* dpos, void* dcls, int N, int Pn, int E, int accumulate);
int valor_sum_over_batch(void* stream, int dtype, const void* x, void* dsum, int N, int Tn, int E, int accumulate);
/* word + position + type embeddings: bert.py:211-215 ; clip.py:377-379 */
int valor_embed_fwd(void* stream, int dtype, const int64_t* ids, const void* word, const void* pos, const void* typevec,
                    void* out, int64_t n, int L, int E);
int valor_embed_bwd_word(void* stream, int dtype, const int64_t* ids, const void* dout, void* dword, int64_t n, int E, int accumulate);
/* decoder inputs: + frame embedding + type embedding, written into the concatenated [video|audio] buffer: modeling.py:485-502 */
int valor_add_frame_type_fwd(void* stream, int dtype, const void* in, const void* frame_emb, const void* type_emb, void* out,
                             int Bn, int F, int X, int E, int64_t out_bs, int64_t out_row_off);
int valor_add_frame_type_bwd(void* stream, int dtype, const void* dout, void* din, void* dframe, float* part, int Bn, int F,
                             int X, int E, int64_t out_bs, int64_t out_row_off);
/* F.normalize(dim=-1): pretrain.py:276,283,290 */
int valor_l2norm_fwd(void* stream, int dtype, const void* x, void* y, float* norm, int64_t rows, int cols);
int valor_l2norm_bwd(void* stream, int dtype, const void* y, const void* dy, const float* norm, void* dx, int64_t rows, int cols);
/* masked-token / cls-token row selection: pretrain.py:441,495 ; modeling.py:387,399. idx[i] < 0 gathers a zero row (and its
 * gradient is dropped by the scatter): VideoSwin window / PatchMerging zero padding, videoswin.py:198-203,222-223,257-259 */
int valor_gather_rows(void* stream, int dtype, const void* src, const int64_t* idx, void* out, int64_t n, int E, int64_t src_ld);
int valor_scatter_rows(void* stream, int dtype, const void* src, const int64_t* idx, void* dst, int64_t n, int E, int64_t dst_ld);
int valor_cast_from_f32(void* stream, int dtype, const float* in, void* out, int64_t n);
/* BERT token masking, modeling.py:134-174, given the per-row mask counts k [b] (int32, 1 <= k[i] <= the row's candidates, drawn by the
 * host: Binomial(m_i, p) | >= 1). Candidates = positions j >= 1 with tokens[i, j] != 0. Each draws Philox4x32-10(seed, offset + i*T + j);
 * the row selects its k[i] candidates with the smallest key w0 | w1 << 32 (ties: lower j); a selected position becomes mask_token if
 * w2 < floor(0.8 * 2^32), else range_start + umulhi(w3, range_end - range_start) if w2 < floor(0.9 * 2^32), else stays (bias of the
 * random token: below (range_end - range_start) / 2^32). tokens_out / labels [b, T] int64, written in full: labels = the original token
 * at selected positions, -1 elsewhere. k[i] is clamped to the row's candidate count. T <= 512; no atomics (deterministic). */
int valor_mask_tokens(void* stream, const int64_t* tokens, const int32_t* k, int b, int T, uint64_t seed, uint64_t offset,
                      int64_t mask_token, int64_t range_start, int64_t range_end, int64_t* tokens_out, int64_t* labels);
/* masked-row gather table of a decoder pass, pretrain.py:441,495 (the order of labels.nonzero()): for every group g < G and every
 * position with labels[i, j] != -1 (row-major), idx[g*n + s] = r0 + (g*b + i)*Ttot + j and lab_out[g*n + s] = labels[i, j], where the
 * selected positions of row i take slots s = row_off[i], row_off[i] + 1, ... (int32 exclusive cumsum of the per-row counts, n = their
 * total). A row never writes past row_off[i + 1] (n for the last row). labels [b, T] int64, T <= 512, Ttot >= T; idx / lab_out [G*n]. */
int valor_masked_rows(void* stream, const int64_t* labels, const int32_t* row_off, int b, int T, int G, int64_t Ttot, int64_t r0,
                      int64_t n, int64_t* idx, int64_t* lab_out);
/* ---- video patch dropout (csrc/patchdrop.hip): every frame keeps k of its Pn patches (+ the class token) in training.
 * valor_patch_keep draws the subsets. Frame f belongs to draw group g = f / group (group = 1: a subset per frame; group = the frames of
 * a clip: one subset per clip, "tube"); N % group == 0. Patch p of group g has the key w0 | w1 << 32 of
 * Philox4x32-10(seed, offset + *rng_base + g*Pn + p) (rng_base: null or ONE device counter read when the kernel runs, as in every dropout
 * entry); the group keeps its k smallest keys, ties to the lower p. idx [N, k] int32: the kept positions of each frame, ascending;
 * slot [N, Pn] int32: the slot of a kept position, -1 for a dropped one. 1 <= k <= Pn <= 1024. The call consumes (N / group) * Pn counters.
 * No atomics: the outputs are a function of the arguments (and *rng_base) alone. */
int valor_patch_keep(void* stream, int N, int Pn, int k, int group, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                     int32_t* idx, int32_t* slot);
/* valor_patchify for the kept patches only: out row f*k + j = patch idx[f, j] of image f (idx [N, k] int32 as valor_patch_keep leaves it;
 * an entry outside 0 .. (H/P)*(W/P) - 1 is clamped). ld_out / pad columns as valor_patchify. */
int valor_patchify_kept(void* stream, int dtype, const float* in, const int32_t* idx, void* out, int N, int C, int H, int W, int P,
                        int k, int64_t ld_out);
/* out [N, 1 + k, E]: out[f][0] = cls + pos[0]; out[f][1 + j] = patches[f*k + j] (+ bias) + pos[1 + idx[f, j]] -- the arithmetic of
 * valor_assemble_tokens_fwd, so the result equals the gathered rows of its output bit for bit. pos [Pn + 1, E]. */
int valor_assemble_tokens_kept_fwd(void* stream, int dtype, const void* patches, const void* cls, const void* pos, const void* bias,
                                   const int32_t* idx, void* out, int N, int Pn, int k, int E);
/* dout [N, 1 + k, E] -> dpatches [N*k, E] = its patch rows; dpos [Pn + 1, E]: row 0 = sum_f dout[f][0] (also to dcls [E] when not null),
 * row 1 + p = sum over the frames with slot[f, p] >= 0 of dout[f][1 + slot[f, p]], in frame order (deterministic; exactly 0 where no
 * frame kept p). accumulate: dpos / dcls += (gradient-arena slots). */
int valor_assemble_tokens_kept_bwd(void* stream, int dtype, const void* dout, const int32_t* slot, void* dpatches, void* dpos, void* dcls,
                                   int N, int Pn, int k, int E, int accumulate);
/* The head of one decoding step against a K|V cache, per sequence r with its new token tok[r] at text position *t_dev (device scalar):
 * x[r, j] = BertEmbeddings before its LayerNorm (bert.py:190-218) of tok[r] at position t (j = 0) and of mask_id at t + 1 (j = 1, J = 2);
 * kmask[r, P + t] = tok[r] != 0 ? 0 : neg (bert.py:857,885); amask [R, J, L] = the step's additive attention rows (causal over the text,
 * bert.py:879-885: slots <= P + t, plus P + t + 1 for the mask row); slots_new[j] = P + t + j. kmask [R, L] fp32 in / out. */
int valor_decode_prologue(void* stream, int dtype, const int64_t* tok, const int64_t* t_dev, const void* word_emb, const void* pos_emb,
                          const void* type_row, int mask_id, int R, int J, int E, int P, int L, float neg, float* kmask, float* amask,
                          void* x, int64_t* slots_new);
/* beam-search selection, VALOR.decode_beam / select (pretrain.py:1080-1098,1156-1159): per sample s the `beam` best of the cur * V
 * candidates  seq_logprob[s, k] + (logits[row, w] - lse[row])  (row = s * row_stride_s + k * row_stride_k; fp32 logits with row pitch ld;
 * lse[row] = the row's log-sum-exp as valor_xent_fwd gives it, or null: computed here and left in lse_out[row] if that is not null),
 * a beam with seq_mask[s, k] == 0 (ended; seq_mask may be null) counting as seq_logprob[s, k] for every w. sel_val / sel_idx: [b, beam],
 * values descending, equal values in index order, idx = k * V + w. beam <= 8. */
int valor_beam_select(void* stream, const float* logits, int64_t ld, int64_t row_stride_s, int64_t row_stride_k, const float* lse,
                      const float* seq_logprob, const float* seq_mask, int b, int cur, int V, int beam, float* sel_val,
                      int64_t* sel_idx, float* lse_out);
/* one step of the beam search with a pool of finished hypotheses (csrc/beam_pool.hip; valor_amd.decode.beam_pool_step_host restates
 * this law on the host, bit for bit): selection, pool update, history reorder and the next step's inputs in one launch. K = beam <= 8,
 * L = max_len <= 512, step t in [0, L). Per sample s (rows of the decoder are beam-major, r = k * b + s; the state is (sample, slot)):
 *   scores_in [b, K] fp32: the summed log-probability c_k of slot k; -inf marks a DEAD slot (a live slot is always above -inf). Only the
 *   slots k < cur are read (cur = 1 at step 0). hist_in / hist_out int64 [b, K, L]: the words so far, a ping-pong pair (never the same
 *   buffer). inv_len fp32 [L + 1]: inv_len[l] = 1 / l^alpha rounded to fp32 by the caller (inv_len[0] = 1); the RANK score of a
 *   hypothesis of summed log-probability c and length l is the fp32 product c * inv_len[l]. The pool, at most K entries per sample:
 *   pool_seq int64 [b, K, L] (padded with eos), pool_logprob / pool_rank fp32 [b, K], pool_len / pool_ins int32 [b, K] (length; insertion
 *   number), pool_cnt int32 [b, 2] = (entries held, insertions so far); the entries held are the slots 0 .. pool_cnt[s, 0] - 1.
 *   done uint8 [b].
 * A sample with done[s] != 0 is frozen: tok = eos, parent = the row itself, scores_out = scores_in, hist_out = hist_in, active = 0, the
 * pool untouched. Otherwise:
 *   1. candidates c(k, w) = scores_in[s, k] + (logits[row, w] - lse[row]) in fp32, in that order, for every live slot k < cur and every
 *      w < V with logits[row, w] > floor; row = s * row_stride_s + k * row_stride_k, row pitch ld, lse[row] the caller's log-sum-exp of
 *      the row (valor_xent_fwd's). floor: -inf, or VALOR_TRIE_FLOOR when valor_trie_constrain masked the rows (a floored column is no
 *      continuation: inside an answer set a sample may run out of open hypotheses, and its pool may hold fewer than K).
 *   2. the 2K best, value descending, equal values in order of the index k * V + w; a candidate equal to -inf (or NaN) is never taken.
 *   3. they are walked in rank order rho = 0, 1, .. until K new slots are filled or the list ends: w == eos offers (words of k + eos, c,
 *      length t + 1) to the pool when rho < K and is skipped otherwise; w != eos fills the next new slot (parent k, token w, score c), and
 *      at t == L - 1 is offered to the pool besides (words of k + w, c, length L).
 *   4. an offer is appended while the pool holds fewer than K entries; a full pool replaces its worst entry -- the lowest rank score,
 *      among equal ones the newest -- only when the offer's rank score is strictly greater.
 *   5. the slots left unfilled are dead: score -inf, token eos, parent = the slot itself.
 *   6. t < L - 1: done[s] = 1 when no new slot was filled, or when the pool holds K entries and (early_stopping != 0 or
 *      worst rank >= c_0 * inv_len[alpha_pos ? L : t + 2], c_0 = the score of new slot 0: the bound of what an open hypothesis can
 *      still reach, exact for log-probabilities <= 0). t == L - 1: done[s] = 1 (the search is over).
 *   7. out: scores_out [b, K]; hist_out[s, j, :] = hist_in[s, parent slot of j, :] with position t = the slot's token; tok / parent
 *      int64 [K * b] beam-major (parent = parent slot * b + s) for the next decoding step; active uint8 [K, b] = the slot is live and
 *      the sample is not done (the rows the next step's valor_logits_constrain / valor_trie_constrain act on).
 * b == 0: no-op. VALOR_ERR_ARG, before any launch: a null pointer, hist_in == hist_out, b < 0, beam outside 1..8, cur outside 1..beam,
 * V < 1, ld < V, a negative row stride, cur * V < 2 * beam or >= 2^31 - 1, max_len outside 1..512, t outside [0, max_len), eos outside
 * [0, V), a NaN floor. One 1024-thread workgroup per sample reads its cur rows once (every thread keeps the best 2K of its stride in registers, then
 * 2K rounds of a workgroup-wide arg max); the walk and the pool update run on one thread, the history and pool rows are copied by all.
 * No atomics, no workspace, vector stores only: the result is a pure function of the inputs, graph replay equals eager issue. */
int valor_beam_pool_step(void* stream, const float* logits, int64_t ld, int64_t row_stride_s, int64_t row_stride_k, const float* lse,
                         const float* scores_in, const int64_t* hist_in, const float* inv_len, int b, int cur, int V, int beam, int max_len,
                         int t, int64_t eos, float floor, int alpha_pos, int early_stopping, float* scores_out, int64_t* hist_out,
                         int64_t* tok, int64_t* parent, uint8_t* active, int64_t* pool_seq, float* pool_logprob, float* pool_rank, int32_t* pool_len,
                         int32_t* pool_ins, int32_t* pool_cnt, uint8_t* done);
/* one step of the DIVERSE (group) beam search with finished-hypothesis pools (csrc/beam_group.hip; valor_amd.decode.beam_group_step_host
 * restates this law on the host, bit for bit): diverse beam search (Vijayakumar et al.) with the Hamming penalty on the current step's
 * words, on top of the pool law above (its rules 1-7 are cited by number). K = beam in 1..8, G = groups divides K, Kg = K / G.
 * pen fp32 [K + 1]: pen[n] = diversity_penalty * n >= 0, the product in fp64 rounded to fp32 once by the caller, pen[0] = 0 (the device
 * does one subtraction and no multiply, so no contraction can differ from the host).
 * State: valor_beam_pool_step's arrays, where group g owns the slots g * Kg .. (g + 1) * Kg - 1 of scores / hist AND the same range of
 * the pool's entries; pool_cnt int32 [b, G, 2] = (entries held, insertions so far) per group; gdone uint8 [b, G]; done uint8 [b].
 * A sample with done[s] != 0 is frozen as rule 7 freezes it. Otherwise its groups are searched in order g = 0 .. G - 1:
 *   1. a group with gdone[s, g] != 0 is frozen exactly as rule 7 freezes a sample (its slots: tok = eos, parent = the row itself,
 *      scores_out = scores_in, hist_out = hist_in, active = 0; its pool range untouched), and it contributes no words to the counts below.
 *   2. otherwise its candidates come from its own live slots k (cur == K), or, at the first step (cur == 1), from the one row of slot 0,
 *      for every group: c(k, w) = scores_in[s, k] + (logits[row, w] - lse[row]) as rule 1, floor included. The SELECTION KEY is
 *      a(k, w) = c(k, w) - pen[n_w], one fp32 subtraction, n_w = the number of NEW OPEN slots that the groups before g filled with word w
 *      at this step (two earlier slots with the same word: pen[2]). eos never fills a slot, so it is never penalised.
 *   3. the 2 Kg best by a, equal keys in order of the index k * V + w (k the slot's index within the sample); a key equal to -inf (or
 *      NaN) is never taken.
 *   4. the walk, the offers and the pool update are rules 3-5 with K -> Kg, on the group's slots and pool range. A new slot carries the
 *      UNPENALISED c and an offer's rank score is c * inv_len[length]: the penalty steers the selection only, scores_out, pool_logprob
 *      and pool_rank stay true (length-ranked) log-probabilities. (HF-style implementations fold the penalty into the running score of
 *      a beam; here a returned score is always the model's own.)
 *   5. rule 6 per group, gdone[s, g] in the place of done[s], the bound taken from the LARGEST c among the group's new slots (under a
 *      penalised order that need not be its first slot). done[s] = 1 when every gdone[s, g] is.
 *   6. out as rule 7; active[k, s] = the slot is live, its group not done (and hence the sample not done).
 * Two identities: G == 1 is valor_beam_pool_step in every array; diversity_penalty == 0 makes every group an independent pool search of
 * beam Kg (all groups then hold the same hypotheses).
 * b == 0: no-op. VALOR_ERR_ARG, before any launch: valor_beam_pool_step's refusals -- cur * V < 2 * beam among them, which at the first
 * step (cur == 1) asks for V >= 2 * beam although a group needs only 2 * Kg candidates -- and groups outside 1..beam or not dividing
 * beam, cur neither 1 nor beam, V < 2 * Kg, a null pen / gdone. One 1024-thread workgroup per sample; the
 * groups run one after another inside the launch (scan of the group's rows with per-thread lists of depth 2 Kg, arg-max rounds, a
 * one-thread walk; the words the earlier groups took are a list of <= 8 in LDS). No atomics, no workspace, vector stores only: the
 * result is a pure function of the inputs. */
int valor_beam_group_step(void* stream, const float* logits, int64_t ld, int64_t row_stride_s, int64_t row_stride_k, const float* lse,
                          const float* scores_in, const int64_t* hist_in, const float* inv_len, const float* pen, int b, int cur, int V,
                          int beam, int groups, int max_len, int t, int64_t eos, float floor, int alpha_pos, int early_stopping,
                          float* scores_out, int64_t* hist_out, int64_t* tok, int64_t* parent, uint8_t* active, int64_t* pool_seq,
                          float* pool_logprob, float* pool_rank, int32_t* pool_len, int32_t* pool_ins, int32_t* pool_cnt, uint8_t* gdone,
                          uint8_t* done);
/* one step of the sampled caption decode, VALOR.decode_greedy mode 'sample' (pretrain.py:1007-1020): per row r < R of fp32 logits
 * [R, V] (row pitch ld >= V) with unfinished[r] != 0, the draw w = argmax_w (z_w - log(-log u_w)) (Gumbel-max: w ~ softmax(z);
 * u_w = (x >> 9) 2^-23 + 2^-24 (exact, in (0, 1)), x = Philox4x32-10(seed, offset + r * ceil(V / 4) + w / 4) word w % 4; ties to the
 * lower index; a -inf logit
 * is never drawn). tok[r] = sents[r * sents_ld] = w, logprobs[r * lp_ld] = z_w - logsumexp(z); unfinished[r] = 0 if w == eos. A row
 * with unfinished[r] == 0 writes eos and logP 0. A row with a NaN logit (or no finite one) writes eos, logP NaN, and finishes.
 * The caller advances offset by R * ceil(V / 4) per step. One workgroup per row, no atomics: deterministic. */
int valor_sample_tokens(void* stream, const float* logits, int64_t ld, int R, int V, uint64_t seed, uint64_t offset, int64_t eos,
                        uint8_t* unfinished, int64_t* tok, int64_t* sents, int64_t sents_ld, float* logprobs, int64_t lp_ld);
/* valor_sample_tokens with temperature, top-k and nucleus (top-p) filters, one launch. Per row r with unfinished[r] != 0:
 *   1. y_w = logits[r, w] * inv_temperature: one rounded fp32 multiply.
 *   2. top-k, when 1 <= top_k < #{w : y_w > -inf}: theta_k = the top_k-th largest y counting duplicates, S_k = {w : y_w >= theta_k}
 *      (more than top_k columns when values tie at theta_k). Otherwise S_k = {w : y_w > -inf}. Exact: integer comparisons only.
 *   3. top-p, when top_p < 1: M = sum over S_k of exp(y_w - max y); walking S_k in descending value, theta_p is the value at which the
 *      running mass first reaches top_p * M; S = {w in S_k : y_w >= theta_p} (never empty: the arg max is always kept). With top_p == 1,
 *      S = S_k. The masses are sums of floor(exp(y_w - max y) * 2^40) in 64-bit integers: independent of the summation order, and the
 *      ratio compared with top_p is within 1e-6 of its exact value, so a boundary closer than that may fall either way.
 *   4. the draw is valor_sample_tokens' on the row where(w in S, y_w, -inf): the same Philox4x32-10 counters offset + r * ceil(V / 4)
 *      + w / 4, word w % 4, indexed by the column of the FULL row (filtering moves no uniform), the same u grid, the same key
 *      y_w - logf(-logf(u_w)), ties to the lower index.
 *   5. logprobs[r * lp_ld] = y_w* - log sum_S exp(y): the log-probability under the distribution drawn from (fp32 statistics).
 *   6. tok / sents / unfinished, rows with unfinished[r] == 0 and rows with a NaN (or no column above -inf) behave as in
 *      valor_sample_tokens. kept[r] = |S| and cut[r] = min over S of y, where the pointers are not NULL; a row that does not draw
 *      (finished before, or NaN) writes kept 0 and cut NaN.
 *   7. inv_temperature == 1, top-k off (0 or >= V) and top_p == 1: tok, sents, logprobs and unfinished are bit-identical to
 *      valor_sample_tokens (that kernel is launched when kept and cut are NULL).
 * R == 0: no-op. VALOR_ERR_ARG, before any launch: a null logits / unfinished / tok / sents / logprobs, R < 0, V < 1 or > 65535 (the
 * bound of the integer masses), ld < V, eos outside [0, V), negative sents_ld / lp_ld / top_k, inv_temperature not finite or <= 0,
 * top_p NaN, <= 0 or > 1. One 1024-thread workgroup per row, 17 KiB of LDS, no workspace, no floating-point atomic: the result does not
 * depend on how the threads split the row, graph replay equals eager issue. The caller advances offset by R * ceil(V / 4) per step. */
int valor_sample_tokens_filtered(void* stream, const float* logits, int64_t ld, int R, int V, uint64_t seed, uint64_t offset, int64_t eos,
                                 float inv_temperature, int top_k, float top_p, uint8_t* unfinished, int64_t* tok, int64_t* sents,
                                 int64_t sents_ld, float* logprobs, int64_t lp_ld, int32_t* kept, float* cut);
/* generation controls of one decoding step, in place on fp32 logits [R, V] (row pitch ld >= V), one launch between the step and the
 * selection (arg max, valor_beam_select, valor_sample_tokens[_filtered]). Row r reads its own generated tokens (prompt and question
 * tokens are not part of it): t int64 ids with unit stride at hist + (r % b) * hist_stride_s + (r / b) * hist_stride_k -- the two
 * strides the way valor_beam_select takes them: beam-major rows r = k * b + s over words kept as [b, beam, max_len] pass
 * hist_stride_s = beam * max_len, hist_stride_k = max_len; a row-ordered history passes b = R, hist_stride_k = 0. t is the same for
 * all rows. Per row r where active is null or active[r] != 0:
 *   1. repetition penalty, when penalty != 1: for every DISTINCT token w of hist[r, 0..t) with 0 <= w < V,
 *      z_w = z_w > 0 ? z_w * inv_penalty : z_w * penalty -- one rounded fp32 multiply, applied once however often w occurs
 *      (inv_penalty = 1 / penalty rounded to fp32 by the caller; -inf stays -inf, +-0 and NaN take the * penalty branch).
 *   2. no repeated n-gram, when ngram = n >= 1 and t >= n - 1: for every i in [0, t - n] with hist[r, i .. i+n-2] ==
 *      hist[r, t-n+1 .. t-1], z_w = -inf for w = hist[r, i+n-1] (n == 1: every token of the history). Overlapping and multiple
 *      matches all count; ids are compared as int64 values.
 *   3. minimum length: when t < min_len, z_eos = -inf.
 *   4. suppressed tokens: z_w = -inf for every w of suppress[0 .. n_suppress) (device int32; duplicates allowed).
 *   Rule 1 runs before the bans: a banned column is -inf whatever rule 1 did to it. Ids outside [0, V), in the history or in the
 *   list, touch no column (in the history they still take part in the n-gram comparison). Columns >= V (the pad of the row), rows
 *   with active[r] == 0 and every column no rule names keep their bits.
 * R == 0: no-op. VALOR_ERR_ARG, before any launch: null logits, null hist with t > 0, R < 0, V < 1, ld < V, t < 0 or > 512 (the
 * history is held in LDS; the decoder has at most 512 positions), b < 1, a negative history stride, ngram < 0, min_len < 0, eos outside
 * [0, V), penalty not finite or <= 0, n_suppress < 0, null suppress with n_suppress > 0. One 256-thread workgroup per row, 4 KiB of
 * LDS, no atomics, no workspace: the result does not depend on how the threads split the history, graph replay equals eager issue. */
int valor_logits_constrain(void* stream, float* logits, int64_t ld, int R, int V, const int64_t* hist, int64_t hist_stride_s,
                           int64_t hist_stride_k, int b, int t, int64_t eos, float penalty, float inv_penalty, int ngram, int min_len,
                           const int32_t* suppress, int n_suppress, const uint8_t* active);
/* closed answer sets: decoding inside a token trie of candidates (csrc/trie.hip). In place on fp32 logits [R, V] (row pitch ld >= V),
 * one launch between the step and the selection, with valor_logits_constrain's history addressing: row r reads t int64 ids with unit
 * stride at hist + (r % b) * hist_stride_s + (r / b) * hist_stride_k, its sample is s = r % b.
 *   The trie, flattened to CSR (valor_amd.decode.AnswerSet builds it): child_ptr int32 [n_nodes + 1]; the children of node i are the
 *   edges child_ptr[i] .. child_ptr[i + 1], child_tok int32 [n_edges] ASCENDING inside a node, child_node int32 [n_edges] the node
 *   behind the edge; terminal uint8 [n_nodes]: a candidate ends at this node; root int32 [n_roots], n_roots = 1 (one set for every
 *   row) or b (a set per sample).
 * Per row r where active is null or active[r] != 0:
 *   1. node = root[n_roots == 1 ? 0 : s];
 *   2. for each of the t history tokens in turn, node = the child of node whose token equals it (compared as int64 values: [SEP], an id
 *      >= V or a negative id simply has no edge), or -1 once there is none;
 *   3. a root or child index outside [0, n_nodes) counts as -1 and is never dereferenced; a child range is clamped to [0, n_edges];
 *   4. the allowed set A = the child tokens of node, plus eos when node == -1 or terminal[node];
 *   5. z_w = VALOR_TRIE_FLOOR for every column w < V that is not in A;
 *   6. the columns in A, the columns >= V (the pad of the row) and the rows with active[r] == 0 keep their bits.
 * The floor is finite: a dead continuation at -inf turns the 0/1-mask arithmetic of the beam search into NaN, and the fused selection
 * never takes a -inf candidate, so a sample with fewer live continuations than beams -- the normal case here -- would leave it without
 * a choice. exp(floor - max) is exactly 0 in fp32 for any row maximum above -1e30 + 104: a floored column has no mass.
 * R == 0: no-op. VALOR_ERR_ARG, before any launch: null logits / child_ptr / terminal / root, null child_tok or child_node with
 * n_edges > 0, null hist with t > 0, R < 0, V < 1, ld < V, t < 0 or > 512, b < 1, a negative history stride, n_roots not 1 or b,
 * n_nodes < 1, n_edges < 0, eos outside [0, V). One 256-thread workgroup per row, 20 KiB of LDS (the history and up to 4096 child
 * tokens; a longer child list is searched in global memory); the row is never read and every column written at most once, with
 * 16-byte stores when logits and ld are multiples of 16 bytes; no atomics, no workspace: the result does not depend on how the threads
 * split the row, graph replay equals eager issue. */
#define VALOR_TRIE_FLOOR (-1e30f)      /* the fp32 nearest to -1e30 (bits 0xF149F2CA) */
int valor_trie_constrain(void* stream, float* logits, int64_t ld, int R, int V, const int64_t* hist, int64_t hist_stride_s,
                         int64_t hist_stride_k, int b, int t, int64_t eos, const int32_t* child_ptr, const int32_t* child_tok,
                         const int32_t* child_node, const uint8_t* terminal, const int32_t* root, int n_nodes, int n_edges, int n_roots,
                         const uint8_t* active);
/* exact scores of a whole closed answer set, one trie LEVEL (or a chunk of one) per launch (csrc/trie.hip): row r = i * b + s of the
 * fp32 logits [rows, V] (row pitch ld >= V, rows = n_level * b) is the decoding step's output after the forced prefix of node
 * level_node[i] (int32 [rows / b], device) for sample s. The trie is valor_trie_constrain's CSR form. In fp32, per row:
 *   1. lse_r = lse[r] when lse is not null (valor_xent_fwd's value); otherwise the row's log-sum-exp computed here while the row is read
 *      once, left in lse_out[r] when that is not null;
 *   2. for every edge e of the node: node_score[child_node[e] * b + s] = node_score[node * b + s] + (z[r, child_tok[e]] - lse_r);
 *   3. if terminal[node]: final[node * b + s] = node_score[node * b + s] + (z[r, eos] - lse_r).
 * The subtraction is rounded first, then the addition. With node_score of the root = 0 (the caller's), levels issued root first,
 * final[node] is the ascending-t fp32 sum of the per-step log-probabilities of the candidate that ends at node: what
 * score_candidates and the beam search assign to it. node_score / final: fp32 [n_nodes * b]; elements the level does not own keep
 * their bits.
 *   A level_node or child_node outside [0, n_nodes) and a child token outside [0, V) are never dereferenced (the arrays live on the
 *   device: they cannot be read before the launch): such a row / edge writes nothing. A child range is clamped to [0, n_edges].
 * rows == 0: no-op. VALOR_ERR_ARG, before any launch: null logits / level_node / child_ptr / terminal / node_score / final, null
 * child_tok or child_node with n_edges > 0, rows < 0 or no multiple of b, more level nodes than n_nodes, V < 1, ld < V, b < 1,
 * n_nodes < 1, n_edges < 0, eos outside [0, V). One 256-thread workgroup per row; 16-byte loads when logits and ld are multiples of 16
 * bytes, 4-byte loads otherwise; the threads stride over the node's edges; every output element is written once, with ordinary
 * vector stores; no atomics, no workspace, the logits are never written: the result does not depend on how the threads split the
 * work. */
int valor_trie_score_level(void* stream, const float* logits, int64_t ld, int64_t rows, int V, int b, const int32_t* level_node,
                           const float* lse, float* lse_out, int64_t eos, const int32_t* child_ptr, const int32_t* child_tok,
                           const int32_t* child_node, const uint8_t* terminal, int n_nodes, int n_edges, float* node_score,
                           float* final);
/* ---- the SCST caption reward on the device: CIDEr-D + BLEU-4 per hypothesis row (csrc/reward.hip; the rules are those of
 * valor_amd/scst.py: scorer/cider_scorer.py:119-200 with n = 1..4 and sigma 6, scorer/bleu_scorer.py:202-250 option 'closest').
 *   KEY of the n-gram (t_0 .. t_{n-1}): (t_i + 1) in bits [16 i, 16 i + 16) of a uint64, unused fields 0 -- exact, n = the number of
 *   non-zero fields. Valid token ids are 0 .. 65533; code 65535 stands for "unknown" and appears in no table.
 *   valor_reward_tables (device pointers; built once per scorer by valor_amd.scst.reward_tables):
 *     g_keys uint64 [n_global] sorted unique, g_idf fp64 [n_global]: every n-gram with a document frequency and its
 *       idf = ref_len - log(max(1, df)), evaluated on the host; an n-gram not in the table has idf = ref_len.
 *     clip_ref_ptr int32 [n_clips + 1]: the references of clip c are clip_ref_ptr[c] .. clip_ref_ptr[c + 1].
 *     ref_key_ptr int32 [#references + 1]; ref_keys uint64 / ref_vals fp64: per reference its sorted unique keys and their tf * idf.
 *     ref_norm fp64 [#references, 4] (the norm per n), ref_bigrams int32 (the count of 2-grams: CIDEr-D's "length"), ref_tokens int32.
 *     clip_bleu_ptr int32 [n_clips + 1]; bleu_keys uint64 sorted unique per clip, bleu_cnt int32: the maximum count over the clip's
 *       references. The lists are trusted (offsets ascending and inside their arrays).
 *   seq int64 [R, L] with row pitch ld >= L (unit column stride), as the sampler and the decoders leave it; clip_idx int32 [R].
 *   Per row: cut at the first eos (tokens behind it never count); a token outside [0, vocab) becomes the unknown code and matches nothing;
 *   hypothesis tf-idf and norms; CIDEr-D = 10 * mean over n and references of the clipped dot product (min(x, y) * y) / both norms (when
 *   neither is 0) * exp(-delta^2 / 72); BLEU-4 = (prod_k (correct_k + 1e-15) / (guess_k + 1e-9))^(1/4), times exp(1 - 1 / ratio) when
 *   ratio = (len + 1e-15) / (closest reference length + 1e-9) < 1 (ties to the shorter reference).
 *   reward fp64 [R] = CIDEr-D + BLEU-4; cider / bleu fp64 [R] receive the two parts where not NULL. A row whose clip_idx is outside
 *   [0, n_clips) or whose clip has no reference gets NaN.
 *   All sums, exp, sqrt and pow are fp64, every reduction has a fixed order and nothing is a floating-point atomic: the same input gives
 *   the same bits. One launch (one workgroup per row) scores any number of rows; nothing is read back. No workspace.
 *   L <= 128: four times the largest max_generation_len any shipped configuration uses. R == 0: no-op. VALOR_ERR_ARG for R < 0, L < 1,
 *   L > 128, ld < L, vocab < 1 or > 65534, eos outside [0, vocab), a null seq / clip_idx / tables / reward or table pointer. */
typedef struct valor_reward_tables {
    const uint64_t* g_keys; const double* g_idf;
    const int32_t* clip_ref_ptr; const int32_t* ref_key_ptr; const uint64_t* ref_keys; const double* ref_vals;
    const double* ref_norm; const int32_t* ref_bigrams; const int32_t* ref_tokens;
    const int32_t* clip_bleu_ptr; const uint64_t* bleu_keys; const int32_t* bleu_cnt;
    double ref_len;
    int32_t n_global, n_clips;
} valor_reward_tables;
int valor_caption_reward(void* stream, const int64_t* seq, int64_t ld, int R, int L, int64_t eos, int vocab, const int32_t* clip_idx,
                         const valor_reward_tables* tables, double* reward, double* cider, double* bleu);
/* ---- caption evaluation on the device: corpus BLEU-1..4, ROUGE-L and CIDEr of one hypothesis per clip (csrc/capeval.hip; the rules
 * are those of valor_amd/capeval.py: cococaption/pycocoevalcap bleu/bleu_scorer.py:201-266 option 'closest', rouge/rouge.py:47-77,
 * cider/cider_scorer.py:96-195). Symbols are small integers (interned words, or model token ids); keys as valor_caption_reward.
 *   valor_capeval_tables (device pointers; built per evaluated clip set by valor_amd.capeval.capeval_tables): the fields of
 *   valor_reward_tables with the same meaning -- the document frequency behind g_idf / ref_vals / ref_norm and ref_len = log(#clips)
 *   are counted over exactly the clips of the table, i.e. the clips being evaluated (pycocoevalcap/eval.py:21) -- plus the references'
 *   raw symbol sequences for the longest common subsequence: ref_sym_ptr int32 [#references + 1], ref_syms uint16 (reference q =
 *   ref_syms[ref_sym_ptr[q] .. ref_sym_ptr[q + 1]), any length). The lists are trusted.
 *   seq int64 [R, L], row pitch ld >= L, L <= 128; a row is cut at its first eos; a symbol outside [0, vocab) matches nothing.
 *   Per row r (all required, they are the input of the corpus reduction; there is no other workspace):
 *     cider fp64 [R]; rouge fp64 [R] = (1 + b^2) P R / (R + b^2 P), b = 1.2, P = max_q lcs_q / len, R = max_q lcs_q / len(ref_q), the two
 *     maxima independent, 0 if either is 0 or the hypothesis is empty; bleu fp64 [R, 4] = the sentence Bleu_1..4 on the row's own integers;
 *     counts int32 [R, 10] = correct[4], guess[4] (guess_k = max(0, len - k + 1)), testlen, the closest reference length (ties: shorter).
 *   summary (a second, one-workgroup launch): value[6] = corpus Bleu_1..4 = (prod_{j<=k} (C_j + 1e-15) / (G_j + 1e-9))^(1/k), times
 *     exp(1 - 1/ratio) when ratio = (T + 1e-15) / (Rl + 1e-9) < 1; the mean ROUGE_L; the mean CIDEr. total[10] = the sums of counts.
 *   A row whose clip_idx is outside [0, n_clips) or whose clip has no reference: NaN in its fp64 outputs, -1 in its counts, all six
 *   summary values NaN (the totals then cover the other rows).
 *   All float arithmetic is fp64, idf and reference tf-idf are the host's bits (no log here), every reduction has a fixed order, the only
 *   atomics are integer ones: the same input gives the same bits.
 *   R == 0: nothing is launched; a non-null summary is set to all zero bytes (values 0.0, totals 0). VALOR_ERR_ARG for R < 0, L < 1,
 *   L > 128, ld < L, vocab < 1 or > 65534, eos outside [0, vocab), a null seq / clip_idx / tables / output / summary or table pointer. */
typedef struct valor_capeval_tables {
    const uint64_t* g_keys; const double* g_idf;
    const int32_t* clip_ref_ptr; const int32_t* ref_key_ptr; const uint64_t* ref_keys; const double* ref_vals;
    const double* ref_norm; const int32_t* ref_bigrams; const int32_t* ref_tokens;
    const int32_t* clip_bleu_ptr; const uint64_t* bleu_keys; const int32_t* bleu_cnt;
    const int32_t* ref_sym_ptr; const uint16_t* ref_syms;
    double ref_len;
    int32_t n_global, n_clips;
} valor_capeval_tables;
typedef struct valor_capeval_summary {
    double value[6];
    int64_t total[10];
} valor_capeval_summary;
int valor_caption_metrics(void* stream, const int64_t* seq, int64_t ld, int R, int L, int64_t eos, int vocab, const int32_t* clip_idx,
                          const valor_capeval_tables* tables, double* cider, double* rouge, double* bleu, int32_t* counts,
                          valor_capeval_summary* summary);
/* backward of a fused activation when no GEMM can absorb it: modeling.py:249-252 */
int valor_dact_mul(void* stream, int dtype, const void* dh, const void* u, void* du, int64_t n, int act);
/* Linear(E -> 1) of the fine-weight heads: pretrain.py:104-112 */
int valor_rowdot_fwd(void* stream, int dtype, const void* x, const void* w, const void* b, void* y, int64_t rows, int cols);
int valor_rowdot_bwd(void* stream, int dtype, const void* dy, const void* x, const void* w, void* dx, void* dw, void* db,
                     int64_t rows, int cols);

/* ---- input preparation on the device (csrc/preproc.hip; the tensor work of AudioMapper / VideoMapper, data/data.py:135-323) ----
 * valor_fbank: kaldi.fbank(htk_compat=True, use_energy=False, window_type='hanning', dither=0) of the selected T-frame slices of B
 * mono clips, padded, normalised and transposed as AudioMapper.__getitem__ returns them: out fp32 [B, A, melbins, T].
 *   wave: the clips packed back to back, n_samples values: fp32 in [-1, 1], or int16 PCM (is_pcm16: the kernel multiplies by 1/32768);
 *   offsets int64 [B + 1] (device): clip b is samples offsets[b] .. offsets[b + 1]; a range that leaves [0, n_samples] makes the clip absent;
 *   slice_idx int32 [B, A] (device): out[b, a] is frames slice_idx*T .. slice_idx*T + T - 1 of the clip's fbank; -1 = no audio: 0.0;
 *   frame f < m = 1 + (N - win) / shift (0 if N < win) is samples f*shift .. f*shift + win - 1: mean removed, pre-emphasis 0.97 with
 *   x[-1] := x[0], times window[win], zero-padded to P (the next power of two >= win, one of 256 / 512 / 1024 / 2048), |FFT|^2, mel sums,
 *   log(max(e, 1.1920929e-07)); frames f >= m are the zero rows of the reference's padding; every value then becomes
 *   (v - mean) / (2 * std);
 *   tables (device, built in fp64 by the caller, valor_amd/preprocess.py fbank_tables): window fp64 [win]; twiddle fp64 [P/2, 2] =
 *   (cos, -sin)(2 pi k / P); filter j sums mel_w[mel_ptr[j] .. mel_ptr[j + 1]) times the power of bins mel_start[j], mel_start[j] + 1, ...
 *   (mel_start int32 [melbins], mel_ptr int32 [melbins + 1], mel_w fp32 [mel_nnz]; bins >= P/2 are never read). melbins <= 256.
 * Only the A * T selected frames of a clip are computed, in fp64 up to the mel energy (fp32 from the log on). Deterministic (no atomics). */
int valor_fbank(void* stream, const void* wave, int is_pcm16, int64_t n_samples, const int64_t* offsets, const int32_t* slice_idx,
                int B, int A, int win, int shift, int P, int melbins, int T, const double* window, const double* twiddle,
                const int32_t* mel_start, const int32_t* mel_ptr, const float* mel_w, int mel_nnz, float mean, float std, float* out);
/* valor_frames_prepare: F uint8 RGB frames, HWC, packed in pixels[n_bytes] at offsets int64 [F] (device) -> out fp32 [F, 3, R, R].
 * geom int32 [F, 11] (device) per frame: H, W (stored size), top, left, h, w (source box), Hv, Wv (size of the virtual resized image of
 * the box), oy, ox (where the R x R output window sits in it), flip. Output pixel (y, x) is the bilinear sample (align_corners=False;
 * antialias != 0: the triangle filter of support max(scale, 1), as torch.nn.functional.interpolate(antialias=True)) of the box at
 * virtual position (y + oy, x + ox), scales h / Hv and w / Wv, taps clamped inside the box; / 255, (v - mean[c]) / std[c], column
 * mirrored if flip. mean / std: HOST pointers to 3 floats. Frames of different stored sizes share one launch; a geometry row or an
 * offset that leaves the buffer reads nothing and makes that frame NaN. Weights and sums are fp64: one rounding, at the store. */
int valor_frames_prepare(void* stream, const uint8_t* pixels, int64_t n_bytes, const int64_t* offsets, const int32_t* geom, int F,
                         int R, int antialias, const float* mean, const float* std, float* out);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Device loss meter (valor_amd/train.py LossMeter): running statistics of the scalars of a training step, no read-back.
 * valor_meter_update: table fp32 [rows, VALOR_METER_FIELDS] (device, 16-byte aligned), one row per metered scalar:
 *   [last, ema, sum, count, min, max, nonfinite, reserved (0)], initialised by the host to [0, 0, 0, 0, +inf, -inf, 0, 0].
 *   src: HOST array of n DEVICE pointers to fp32 scalars; row_of: HOST array of n row indices. Both travel as kernel arguments (no copy,
 *   nothing of them is read after the call returns). One launch of one wave, lane i owns source i. For x = *src[i], r = row_of[i]:
 *   last = x always; x not finite: nonfinite += 1, nothing else changes; otherwise ema = count == 0 ? x : x * take + ema * keep (each
 *   product and the sum rounded on its own: no FMA), sum += x, count += 1, min = fminf(min, x), max = fmaxf(max, x). count and nonfinite
 *   are fp32 counters (exact up to 2^24 updates of a row).
 *   n == 0: no-op. VALOR_ERR_ARG before any launch: n outside [0, VALOR_METER_MAX_SRC], rows < 1, a null table / src / row_of or entry
 *   of src, a table that is not 16-byte or a source that is not 4-byte aligned, a row index outside [0, rows), two sources on one row. */
#define VALOR_METER_FIELDS 8
#define VALOR_METER_MAX_SRC 32
int valor_meter_update(void* stream, float* table, int rows, const float* const* src, const int32_t* row_of, int n,
                       float keep, float take);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Training diagnostics (valor_amd/diagnostics.py): statistics per arena tensor and per optimizer group, computed on the device around
 * the fused update, no read-back; nothing that is trained is written. They take the arenas and tables of valor_adamw_counted --
 * chunk_group int8 [n/chunk] (-1 = inactive this step), chunk_tensor int32 [n/chunk], chunk_bc as valor_adamw_counted left it, the device
 * gscale -- and tensor_numel int64 [ntensors] (device): tensor t occupies ceil(tensor_numel[t] / chunk) consecutive chunks and ONLY its
 * tensor_numel[t] elements count; the padding behind its tail is never read into a statistic (it may hold NaN).
 *   tensor_stats fp32 [ntensors, VALOR_STATS_FIELDS], group_stats fp32 [ngroups, VALOR_STATS_FIELDS] (device, 16-byte aligned); a row:
 *     0 g_sumsq      sum of g^2 over the FINITE elements, unscaled        4 w_sumsq  sum of w^2 (fp32 master)
 *     1 g_absmax     max |g| over the finite elements                     5 u_sumsq  sum of u^2, u = lr_g * bc[1] / bc[0] * m / (sqrtf(v) + eps)
 *     2 g_nonfinite  number of inf / NaN elements (fp32 counter)          6 w_norm   sqrt(w_sumsq)
 *     3 g_norm       sqrt(g_sumsq) * norm_mul (units of total_norm)       7 u_ratio  sqrt(u_sumsq) / (w_norm + 1e-12)
 *   valor_arena_grad_stats (between valor_grad_norm_clip and the update, which clears the gradients) writes fields 0-3 of every row;
 *   valor_arena_update_stats (behind the update) writes fields 4-7: u is the Adam term the update has just applied, from the moments
 *   behind the step, without the decay term; lr: HOST array of ngroups floats. A non-finite *gscale_dev (the step was skipped) makes
 *   fields 5 and 7 zero in every row; gscale_dev may be null. An inactive tensor has zeros in the fields of the call. A group row is the
 *   fold of its active tensors in tensor-index order: sum, max, sum of the tensor rows, norm and ratio recomputed from the folded sums.
 *   Deterministic (no floating-point atomics; per-chunk partials in scratch, a tensor's chunks reduced in a fixed order of their own, in
 *   fp64): two calls on the same data give the same bits and a tensor's row does not depend on which other tensors are active. A sum
 *   of squares is within 23 fp32 ulp (1.4e-6 relative) of exact arithmetic plus the roundings of the stored rows, whatever the size.
 *   scratch: fp32 words, 16-byte aligned, >= 4 * n/chunk + 2 * (ntensors rounded up to 4). Three launches each, one read of every arena.
 *   n == 0: no-op. VALOR_ERR_ARG before any launch: a null pointer (but gscale_dev), n < 0 or not a multiple of valor_adamw_chunk(),
 *   ntensors < 1, ngroups outside [1, 16], an unknown dtype, an arena / scratch / stats table that is not 16-byte aligned, chunk_tensor
 *   not 4-byte, tensor_numel / chunk_bc not 8-byte, gscale_dev not 4-byte aligned. */
#define VALOR_STATS_FIELDS 8
int valor_arena_grad_stats(void* stream, int dtype, const void* grad, const int8_t* chunk_group, const int32_t* chunk_tensor,
                           const int64_t* tensor_numel, int ntensors, int64_t n, int ngroups, float norm_mul, float* scratch,
                           float* tensor_stats, float* group_stats);
int valor_arena_update_stats(void* stream, const float* master, const float* exp_avg, const float* exp_avg_sq,
                             const int8_t* chunk_group, const int32_t* chunk_tensor, const float* chunk_bc,
                             const int64_t* tensor_numel, int ntensors, int64_t n, const float* lr, int ngroups, float eps,
                             const float* gscale_dev, float* scratch, float* tensor_stats, float* group_stats);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Exponential moving average of the weights (valor_amd/ema.py WeightEMA): one streaming pass over the fp32 masters, no read-back.
 * valor_ema_update: w fp32 [n] (the masters, read only), ema fp32 [n] (updated in place), count: ONE device int32, the number of updates
 *   applied so far; decay and warmup are host scalars. Per element, in fp32, every named operation rounded once (no FMA contraction, so
 *   a restatement in plain fp32 tensor operations is bit-equal):
 *     k = *count ;  d = warmup ? min(decay, (1 + k) / (10 + k)) : decay   (one IEEE division of the two integers converted to fp32)
 *     a = 1 - d ;  t = w - ema ;  ema = ema + a * t                        (a product, then a sum)
 *   so an element with w == ema stays exactly where it is, whatever d. Afterwards *count advances by one (a second, one-thread launch
 *   behind the first, as valor_adamw_counted's). A non-finite *gscale_dev (the optimizer skipped the step; gscale_dev may be null)
 *   writes nothing and leaves the count: the test valor_adamw* apply. Any n > 0 (the last n % 4 elements are a scalar tail); pads of an
 *   arena are ordinary elements. 12 bytes of memory traffic per element. Two launches, deterministic.
 *   VALOR_ERR_ARG before any launch: a null w / ema / count, n <= 0, decay outside [0, 1] or NaN, w or ema not 16-byte aligned, count or
 *   gscale_dev not 4-byte aligned, w and ema overlapping. */
int valor_ema_update(void* stream, const float* w, float* ema, int64_t n, float decay, int warmup, int32_t* count,
                     const float* gscale_dev);
/* non-temporal accesses of valor_ema_update (bit 0 loads, bit 1 stores; A/B hook, env VALOR_EMA_NT); returns the previous value, v < 0 queries */
int valor_ema_set_nt(int v);

#ifdef __cplusplus
}
#endif
#endif /* VALOR_HIP_H */
