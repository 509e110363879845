"""Retrieval search: a clip bank that stays on the device and answers text queries with the k best clips (validate_ret needs ground
truth, builds the whole [texts, clips] matrix and returns recall numbers; this is the path a user of a retrieval model runs).

RetrievalIndex.build / add encode gallery batches with the text side off and keep what the text -> clip score of validate_ret reads:
  contra_type 'fine'    token features [NB, Nv, D] in the model's dtype ([video | audio] along the token axis for 'tva') and their
                        softmaxed token weights [NB, Nv] (raw fine_weight_mapper outputs concatenated, then valor_fine_weight_softmax,
                        as validate_ret builds them; the clip mask is all ones and stays implicit). late_fusion keeps a video and an
                        audio bank with unit token weights and adds the two scores (test.py:571-579).
  contra_type 'coarse'  pooled vectors [NB, D] (after va_fusion for 'tva'; late_fusion: both banks, the scores added).
search() encodes the queries by the text path only and walks the bank in chunks: a chunk's [NQ, chunk] fp32 scores come from the
kernels evaluate.fine_score_matrix uses (valor_fine_fused_fwd for bf16 features, the fp32 GEMM + valor_fine_scores otherwise; K.gemm
for coarse) and are folded into the running [NQ, k] result by valor_topk_rows(merge=1, col_base=chunk start) (csrc/search.hip). Nothing
of size [NQ, NB] exists, and nothing comes back to the host before the caller reads `.ids`.

bank_dtype="fp8" (fine banks only, opt-in; csrc/search_fp8.hip): the bank keeps OCP e4m3 codes [NB, Nv, D] (uint8) and one fp32 scale per
token row [NB, Nv] instead of the features -- half the bytes of a bf16 bank. build / add / from_features / quantize() encode the
incoming rows with valor_fp8_quantize_rows; search() quantises the query rows per call with the same kernel and scores a chunk with
valor_fine_fused_fwd_fp8 (the e4m3 MFMA form of valor_fine_fused_fwd, scores only). The quantisation law and the score law are restated
on the host below (quantize_rows_host, fp8_scores_host). An index built without bank_dtype is what it was.

bank_dtype="mxfp4" (fine banks only, opt-in; csrc/search_mx.hip): the bank keeps OCP MX e2m1 codes [NB, Nv, D / 2] (two elements per
byte, element 2i in the low nibble) and one E8M0 scale byte per block of 32 elements [NB, Nv, D / 32] -- D / 2 + D / 32 bytes per token
row, a little over half of an fp8 bank. Rows are encoded by valor_mx_quantize_rows (the OCP MX v1.0 conversion); search() quantises the
query rows per call to MX e4m3 with the same kernel and scores a chunk with valor_fine_fused_fwd_mx, whose block-scaled MFMA takes
the two formats and applies both scales in hardware. fp4 scores are coarse: the answer a user wants comes from the exact store and the
two-stage search below, which an mxfp4 bank has exactly as an fp8 bank has them. The laws are restated on the host
(mx_quantize_rows_host, mx_dequantize_host, mx_scores_host).

Pair scores (csrc/search_pairs.hip): valor_fine_score_pairs scores every query against ITS OWN list of clips, read by index from a bf16
feature store (score_pairs; the law restated in fp64 by pair_scores_host). Three things stand on it:
  rescore(model, queries, candidates)   the exact scores [NQ, C] of given bank indices (-1 allowed: -inf).
  search(..., within=candidates)        the k best of each query's candidate list, in the search's one total order (score descending,
                                        then bank index ascending): the rows are sorted ascending and de-duplicated on the device,
                                        the pairs scored, valor_topk_rows selects, positions map back. Nothing of size [NQ, NB].
  exact="device" | "host" (fp8 banks)   the bf16 features the codes were made from are kept too, on the device or in pinned host
                                        memory, and search(..., shortlist=k') becomes a two-stage search: the fp8 walk returns k'
                                        candidates, they are re-scored on the exact features, the exact top k is returned with the
                                        exact scores. shortlist=0 (and every index without a store) is the fp8-only search.

Pair alignments (csrc/search_align.hip): valor_fine_align_pairs keeps what the pair score reduces away -- per pair the maxima of either
direction, their first arg maxima, the score split over the text tokens and over the clip tokens (the credits), and on request the
masked token similarities (align_pairs; the law restated by align_pairs_host / credits_host). explain(model, queries, candidates)
returns them as an Alignment for given bank indices, search(..., explain=True) attaches one for exactly the returned indices; the
scores and indices of the search are untouched. `token_layout` names the modality of every clip token, so the clip credits can be
summed per modality (Alignment.clip_credit_by_modality) and the best clip token named (Alignment.best_clip_token).

Removal, filters, groups (csrc/search_select.hip): valor_topk_rows_select is valor_topk_rows with a keep byte and a group id per
candidate (topk_rows_select; the law restated by topk_select_host). Three things stand on it:
  remove(ids= | indices=)               tombstones clips in a device bool array: no search path returns them again; positions keep
                                        their meaning, compact() rewrites every store without them and returns the old -> new map,
                                        update() is remove + add_features.
  search(..., where=mask)               only the clips a device bool mask admits ([NB], or [NQ, NB] per query), ANDed with the alive array.
  groups= / search(..., collapse=True)  one hashable label per clip (the video a segment was cut from); collapse returns one clip per
                                        group, the group's best admitted one. A two-stage search filters in its first stage and
                                        collapses in the second, on the exact scores.
An index that removed nothing, has no groups and gets no where= runs valor_topk_rows, as it did.

Out of scope: dual_softmax (it needs the whole matrix), the va / vta / atv directions, a bank sharded over GPUs,
attribute predicates evaluated on the device (the caller builds the mask), more than one result per group, a collapsing first stage,
approximate search, a coarse first stage, kernel reads of host memory (the host store is gathered and copied), fp32 or
coarse pair scores; for fp8 and mxfp4 banks also coarse banks (they need a GEMM of their own) and quantised codes anywhere in
validate_ret or training; e2m1 queries and MX-e4m3 or fp6 banks (the kernel's format arguments would allow them); alignments on coarse
banks or straight on codes, the clip -> text direction, word strings, span selection."""
import ctypes

import torch

from . import evaluate as E
from . import kernels as K
from . import lib, ops

GROUPS = ("tv", "tva", "ta")
_GEMM_PATH_BYTES = 1 << 30          # the fp32 token-similarity buffer of the non-fused fine path, per chunk


# ------------------------------------------------------------------ the kernel's law on the host (checks only)
def topk_host(score, k, base=0, state=None):
    """What valor_topk_rows computes, restated with stable sorts: score [R, C]; the candidates of a row are (score[r, c], base + c) and,
    with state = (val [R, k], idx [R, k]), the state's entries of index >= 0. Value descending, then index ascending, NaN below every
    number; missing candidates are -inf / -1. Returns (val fp32 [R, k], idx int64 [R, k]) on the CPU."""
    score = score.detach().float().cpu()
    R, C = score.shape
    val = score
    idx = (torch.arange(C, dtype=torch.int64) + base)[None].expand(R, C)
    valid = torch.ones((R, C), dtype=torch.bool)
    if state is not None:
        sv, si = state[0].detach().float().cpu(), state[1].detach().long().cpu()
        val, idx, valid = torch.cat((sv, val), 1), torch.cat((si, idx), 1), torch.cat((si >= 0, valid), 1)
    pad = max(0, k - val.shape[1])
    if pad:
        val = torch.cat((val, torch.zeros((R, pad))), 1)
        idx = torch.cat((idx, torch.full((R, pad), -1, dtype=torch.int64)), 1)
        valid = torch.cat((valid, torch.zeros((R, pad), dtype=torch.bool)), 1)
    nan = torch.isnan(val)
    klass = torch.where(valid, nan.long(), torch.full_like(idx, 2))                 # numbers, then NaNs, then nothing
    key = torch.where(nan | ~valid, torch.full_like(val, float("-inf")), val)
    # least significant key first, every sort stable: index ascending, value descending, class ascending
    order = torch.sort(idx, dim=1, stable=True)[1]
    order = order.gather(1, torch.sort(key.gather(1, order), dim=1, descending=True, stable=True)[1])
    order = order.gather(1, torch.sort(klass.gather(1, order), dim=1, stable=True)[1])[:, :k]
    ok = valid.gather(1, order)
    out_v = torch.where(ok, val.gather(1, order), torch.full((R, k), float("-inf")))
    out_i = torch.where(ok, idx.gather(1, order), torch.full((R, k), -1, dtype=torch.int64))
    return out_v, out_i


def topk_rows(score, k, col_base=0, state=None, workspace=None):
    """valor_topk_rows on a device fp32 matrix [R, C] (unit column stride). state = (top_val fp32 [R, k], top_idx int64 [R, k]) is
    updated in place (merge); without it a fresh pair is returned."""
    K._check_gpu(score)
    if score.dtype != torch.float32 or score.dim() != 2 or score.stride(1) != 1:
        raise ValueError("score: an fp32 [rows, columns] matrix with unit column stride")
    R, C = score.shape
    merge = state is not None
    if merge:
        top_val, top_idx = state
        K._check_gpu(top_val, top_idx)
        if (tuple(top_val.shape) != (R, k) or tuple(top_idx.shape) != (R, k) or top_val.dtype != torch.float32 or top_idx.dtype != torch.int64
                or not top_val.is_contiguous() or not top_idx.is_contiguous()):
            raise ValueError(f"state: contiguous fp32 / int64 [{R}, {k}] tensors")
    else:
        top_val = torch.empty((R, k), dtype=torch.float32, device=score.device)
        top_idx = torch.empty((R, k), dtype=torch.int64, device=score.device)
    need = topk_workspace_bytes(R, C, k)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=score.device)
    lib.call("valor_topk_rows", K._stream(), score.data_ptr(), score.stride(0) if R > 1 else max(score.stride(0), C), R, C, int(col_base), int(k),
             int(merge), top_val.data_ptr(), top_idx.data_ptr(), workspace.data_ptr(), workspace.numel())
    return top_val, top_idx


def topk_workspace_bytes(R, C, k):
    n = ctypes.c_int64()
    lib.call("valor_topk_workspace_bytes", int(R), int(C), int(k), ctypes.byref(n))
    return n.value


def topk_select_host(score, k, base=0, state=None, keep=None, group=None):
    """What valor_topk_rows_select computes, restated with stable sorts: topk_host's candidates and order, and
    keep  (bool / uint8 [N] for all rows or [R, N]; None: all): the candidate of index i is eligible iff keep[..., i] != 0 -- the
          state's entries are checked like the columns';
    group (integer [N] or [R, N]; None: no grouping): the eligible candidates of one id g >= 0 are one result, represented by the
          first of them in sorted order; g < 0 is a group of its own. The k best representatives are returned.
    With both None this is topk_host. Returns (val fp32 [R, k], idx int64 [R, k]) on the CPU."""
    score = score.detach().float().cpu()
    R, C = score.shape
    val = score
    idx = (torch.arange(C, dtype=torch.int64) + base)[None].expand(R, C)
    valid = torch.ones((R, C), dtype=torch.bool)
    if state is not None:
        sv, si = state[0].detach().float().cpu(), state[1].detach().long().cpu()
        val, idx, valid = torch.cat((sv, val), 1), torch.cat((si, idx), 1), torch.cat((si >= 0, valid), 1)
    pad = max(0, k - val.shape[1])
    if pad:
        val = torch.cat((val, torch.zeros((R, pad))), 1)
        idx = torch.cat((idx, torch.full((R, pad), -1, dtype=torch.int64)), 1)
        valid = torch.cat((valid, torch.zeros((R, pad), dtype=torch.bool)), 1)
    N = val.shape[1]
    at = lambda table: (table[None].expand(R, -1) if table.dim() == 1 else table).gather(1, idx.clamp(min=0))
    if keep is not None:
        valid = valid & (at(keep.detach().cpu()) != 0)
    gid = at(group.detach().cpu().long()) if group is not None else torch.full((R, N), -1, dtype=torch.int64)
    nan = torch.isnan(val)
    klass = torch.where(valid, nan.long(), torch.full_like(idx, 2))                 # numbers, then NaNs, then nothing
    key = torch.where(nan | ~valid, torch.full_like(val, float("-inf")), val)
    # least significant key first, every sort stable: index ascending, value descending, class ascending
    order = torch.sort(idx, dim=1, stable=True)[1]
    order = order.gather(1, torch.sort(key.gather(1, order), dim=1, descending=True, stable=True)[1])
    order = order.gather(1, torch.sort(klass.gather(1, order), dim=1, stable=True)[1])
    ok = valid.gather(1, order)
    # one key per group: the id, or for a candidate on its own (and for nothing) a negative key no other position has. A stable sort
    # by that key puts a group's members side by side in rank order: every member behind the first is a duplicate.
    rank = torch.arange(N, dtype=torch.int64)[None].expand(R, N)
    g = gid.gather(1, order)
    gkey = torch.where(ok & (g >= 0), g, -1 - rank)
    by_group = torch.sort(gkey, dim=1, stable=True)
    later = torch.zeros((R, N), dtype=torch.bool)
    later[:, 1:] = by_group[0][:, 1:] == by_group[0][:, :-1]
    dup = torch.zeros((R, N), dtype=torch.bool).scatter(1, by_group[1], later)
    first = torch.sort(dup.long(), dim=1, stable=True)[1][:, :k]                   # the representatives in rank order, then the rest
    order, ok = order.gather(1, first), ok.gather(1, first) & ~dup.gather(1, first)
    out_v = torch.where(ok, val.gather(1, order), torch.full((R, k), float("-inf")))
    out_i = torch.where(ok, idx.gather(1, order), torch.full((R, k), -1, dtype=torch.int64))
    return out_v, out_i


def _select_table(name, t, dtypes, R, need, device):
    """a keep / group array for valor_topk_rows_select: (tensor, leading dimension); [N] (ld 0) or [R, N], N >= need, unit stride"""
    if (not torch.is_tensor(t) or t.dtype not in dtypes or t.device != device or t.dim() not in (1, 2) or t.shape[-1] < need
            or (t.dim() == 2 and t.shape[0] != R) or (t.shape[-1] > 1 and t.stride(-1) != 1)):
        raise ValueError(f"{name}: a {' / '.join(str(d) for d in dtypes)} tensor [N] or [{R}, N] on {device} with N >= {need} and unit stride")
    return t, (0 if t.dim() == 1 else (t.stride(0) if R > 1 else max(t.stride(0), t.shape[1])))


def topk_rows_select(score, k, col_base=0, state=None, workspace=None, keep=None, group=None, check_state=True):
    """valor_topk_rows_select: topk_rows with keep (bool / uint8 [N] or [R, N], indexed by col_base + column) and group (int32, same
    shapes); either may be None. THE TABLES ARE ADDRESSED BY INDEX, NOT BY COLUMN: they must cover col_base + C entries AND every index
    the state holds, because the merge reads keep / group of the state's entries too -- tables cut to the current chunk are an
    out-of-bounds read on the device. Both are checked here and raise ValueError; the state's largest index costs one read-back, which
    check_state=False leaves out for a caller whose tables cover everything it folds (RetrievalIndex: they span the bank)."""
    K._check_gpu(score)
    if score.dtype != torch.float32 or score.dim() != 2 or score.stride(1) != 1:
        raise ValueError("score: an fp32 [rows, columns] matrix with unit column stride")
    R, C = score.shape
    merge = state is not None
    if merge:
        top_val, top_idx = state
        K._check_gpu(top_val, top_idx)
        if (tuple(top_val.shape) != (R, k) or tuple(top_idx.shape) != (R, k) or top_val.dtype != torch.float32 or top_idx.dtype != torch.int64
                or not top_val.is_contiguous() or not top_idx.is_contiguous()):
            raise ValueError(f"state: contiguous fp32 / int64 [{R}, {k}] tensors")
    else:
        top_val = torch.empty((R, k), dtype=torch.float32, device=score.device)
        top_idx = torch.empty((R, k), dtype=torch.int64, device=score.device)
    keep, keep_ld = (None, 0) if keep is None else _select_table("keep", keep, (torch.bool, torch.uint8), R, int(col_base) + C, score.device)
    group, group_ld = (None, 0) if group is None else _select_table("group", group, (torch.int32,), R, int(col_base) + C, score.device)
    if merge and check_state and (keep is not None or group is not None) and k:
        held, covered = int(top_idx.max()), min(t.shape[-1] for t in (keep, group) if t is not None)
        if held >= covered:
            raise ValueError(f"the state holds index {held}, the keep / group tables cover {covered} entries: size them for every index folded so far")
    need = topk_select_workspace_bytes(R, C, k)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=score.device)
    lib.call("valor_topk_rows_select", K._stream(), score.data_ptr(), score.stride(0) if R > 1 else max(score.stride(0), C), R, C, int(col_base),
             int(k), int(merge), None if keep is None else keep.data_ptr(), keep_ld, None if group is None else group.data_ptr(), group_ld,
             top_val.data_ptr(), top_idx.data_ptr(), workspace.data_ptr(), workspace.numel())
    return top_val, top_idx


def topk_select_workspace_bytes(R, C, k):
    n = ctypes.c_int64()
    lib.call("valor_topk_select_workspace_bytes", int(R), int(C), int(k), ctypes.byref(n))
    return n.value


# ------------------------------------------------------------------ the fp8 bank's laws on the host (checks only)
BANK_DTYPES = (None, "fp8", "mxfp4")
_QUANTISED = ("fp8", "mxfp4")                                         # banks kept as codes and scales
_SCORE_KERNEL = {"fp8": "valor_fine_fused_fwd_fp8", "mxfp4": "valor_fine_fused_fwd_mx"}
_FP8_MAX, _FP8_TINY = 448.0, 2.0 ** -64


def quantize_rows_host(x):
    """What valor_fp8_quantize_rows computes, restated on the CPU: x [..., D] -> (uint8 e4m3fn codes [..., D], fp32 scales [...]). All
    in fp32: amax = max |x|; amax < 2^-64: scale 0, codes 0x00; else scale = amax / 448, inv = 448 / amax, code = e4m3fn(clamp(x * inv,
    -448, 448)) (torch's CPU conversion: round to nearest even, subnormals and sign kept; the clamp keeps it away from NaN)."""
    x = x.detach().float().cpu()
    amax = x.abs().amax(-1, keepdim=True)
    live = amax >= _FP8_TINY
    safe = torch.where(live, amax, torch.ones_like(amax))
    scale = torch.where(live, safe / _FP8_MAX, torch.zeros_like(amax))
    # a tensor / tensor division: `448.0 / safe` would be reciprocal-then-multiply, two roundings, and bf16 inputs put many products
    # x * inv exactly on e4m3 ties, where the last bit of inv decides the code
    inv = torch.where(live, torch.full_like(amax, _FP8_MAX) / safe, torch.zeros_like(amax))
    codes = (x * inv).clamp(-_FP8_MAX, _FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return torch.where(live, codes, torch.zeros_like(codes)), scale.squeeze(-1)


def fp8_scores_host(codesA, scaleA, codesB, scaleB, maskA, maskB, wA, wB):
    """What valor_fine_fused_fwd_fp8 computes, in fp64 on the CPU: compute_fine_matrix_slice (pretrain.py:191-211) on the dequantised
    rows. codesA uint8 [NA, T, D], scaleA [NA, T], codesB [NB, Nv, D], scaleB [NB, Nv], masks and SOFTMAXED token weights [NA, T] /
    [NB, Nv]. sim = scaleA scaleB sum_d codeA codeB; x = sim maskA maskB; score = (sum_t wA max_v x + sum_v wB max_t x) / 2. [NA, NB] fp64."""
    f64 = lambda t: t.detach().cpu().double()
    de = lambda c: c.detach().cpu().view(torch.float8_e4m3fn).float().double()
    sA, sB, mA, mB = f64(scaleA), f64(scaleB), f64(maskA), f64(maskB)
    sim = torch.einsum("atd,bvd->abtv", de(codesA), de(codesB)) * sA[:, None, :, None] * sB[None, :, None, :]
    x = sim * mA[:, None, :, None] * mB[None, :, None, :]
    return (torch.einsum("abt,at->ab", x.max(dim=3)[0], f64(wA)) + torch.einsum("abv,bv->ab", x.max(dim=2)[0], f64(wB))) / 2.0


def quantize_rows(x):
    """valor_fp8_quantize_rows on device bf16 / fp32 rows x [..., D] (D % 16 == 0; a 2-D x may be a column slice of a wider matrix):
    (uint8 codes [..., D] dense, fp32 scales [...]). A non-finite value raises ValueError (one isfinite reduction on the device, read
    back by the host: bank rows and query rows alike, the law is undefined on such rows)."""
    K._check_gpu(x)
    if x.dtype not in (torch.bfloat16, torch.float32) or x.dim() < 1 or x.shape[-1] % 16 or x.shape[-1] == 0:
        raise ValueError(f"quantize_rows: bf16 or fp32 rows of a multiple of 16 elements, got {tuple(x.shape)} {x.dtype}")
    cols = x.shape[-1]
    strided = x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= cols and (x.stride(0) * x.element_size()) % 16 == 0 and x.data_ptr() % 16 == 0
    if not strided:
        x = x.contiguous()
    if not bool(torch.isfinite(x).all()):
        raise ValueError("quantize_rows: the rows hold a non-finite value")
    rows = x.numel() // cols
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    scales = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    lib.call("valor_fp8_quantize_rows", K._stream(), 0 if x.dtype == torch.bfloat16 else 1, x.data_ptr(), x.stride(0) if strided else cols, rows,
             cols, codes.data_ptr(), scales.data_ptr())
    return codes, scales


def _scores_fp8(qc, qs, bc, bs, maskA, maskB, wA, wB, out):
    """out [NA, nb] (dense fp32) = valor_fine_fused_fwd_fp8 on contiguous codes / scales, the A rows in pieces under the kernel's byte limit"""
    NA, T, D = qc.shape
    nb, Nv = bc.shape[:2]
    st = K._stream()
    ra = max(1, min(NA, (E._FUSED_BYTES - 1) // (T * D)))
    for a0 in range(0, NA, ra):
        na = min(ra, NA - a0)
        lib.call("valor_fine_fused_fwd_fp8", st, qc[a0:a0 + na].data_ptr(), qs[a0:a0 + na].data_ptr(), bc.data_ptr(), bs.data_ptr(),
                 maskA[a0:a0 + na].data_ptr(), maskB.data_ptr(), wA[a0:a0 + na].data_ptr(), wB.data_ptr(), out[a0:a0 + na].data_ptr(), na, nb, T, Nv, D)
    return out


# ------------------------------------------------------------------ the mxfp4 bank's laws on the host (checks only) and the wrappers
MX_E4M3, MX_E2M1 = lib.MX_E4M3, lib.MX_E2M1                           # VALOR_MX_*: the hardware's format ids
_MX_FORMATS = {MX_E4M3: (8, 448.0), MX_E2M1: (2, 6.0)}                # format -> (emax, largest magnitude)
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)                # the magnitude of every e2m1 code; bit 3 is the sign


def _mx_format(fmt):
    if fmt not in _MX_FORMATS:
        raise ValueError(f"fmt {fmt!r}: MX_E4M3 ({MX_E4M3}) or MX_E2M1 ({MX_E2M1})")
    return _MX_FORMATS[fmt]


def mx_quantize_rows_host(x, fmt):
    """What valor_mx_quantize_rows computes, restated on the CPU (the OCP MX v1.0 conversion): x [..., D], D % 32 == 0 -> (uint8 codes
    [..., D] for MX_E4M3 / [..., D / 2] for MX_E2M1, element 2i in the low nibble of byte i; uint8 E8M0 scale bytes [..., D / 32]). Per
    block of 32: amax = max |x|, e = the fp32 exponent field of amax - 127 (floor(log2 amax); zero and subnormal amax: -127),
    s = max(e - emax, -127), byte = s + 127, code = RNE(clamp(x * 2^-s, -max, max)) -- the product is formed exactly (in fp64), ties go
    to the even code, the sign of zero and the element format's subnormals are kept."""
    emax, vmax = _mx_format(fmt)
    x = x.detach().float().cpu().contiguous()
    D = x.shape[-1]
    if D % 32 or D == 0:
        raise ValueError(f"mx_quantize_rows_host: rows of a multiple of 32 elements, got {tuple(x.shape)}")
    blk = x.reshape(x.shape[:-1] + (D // 32, 32))
    amax = blk.abs().amax(-1).contiguous()
    e = ((amax.view(torch.int32) >> 23) & 0xff) - 127
    s = (e - emax).clamp(min=-127)                                       # the upper clamp (127) is out of a finite fp32's reach
    mul = ((127 - s) << 23).to(torch.int32).view(torch.float32)          # 2^-s, built from its bits
    y = (blk.double() * mul.double()[..., None]).clamp(-vmax, vmax)
    if fmt == MX_E4M3:
        codes = y.float().to(torch.float8_e4m3fn).view(torch.uint8).reshape(x.shape)
    else:
        m = y.abs()
        # seven compares at the midpoints of 0, .5, 1, 1.5, 2, 3, 4, 6: `>` where the lower neighbour has the even code, `>=` otherwise
        c = sum(((m > t) if strict else (m >= t)).to(torch.uint8)
                for t, strict in ((0.25, True), (0.75, False), (1.25, True), (1.75, False), (2.5, True), (3.5, False), (5.0, True)))
        c = (c | (torch.signbit(blk).to(torch.uint8) << 3)).reshape(x.shape[:-1] + (D // 2, 2))
        codes = c[..., 0] | (c[..., 1] << 4)
    return codes.contiguous(), (s + 127).to(torch.uint8)


def mx_dequantize_host(codes, scales, fmt):
    """The values MX codes stand for, fp64 [..., D] on the CPU: element * 2^(scale byte - 127)."""
    _mx_format(fmt)
    codes, scales = codes.detach().cpu().contiguous(), scales.detach().cpu()
    if fmt == MX_E4M3:
        el = codes.view(torch.float8_e4m3fn).float().double()
    else:
        nib = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(codes.shape[:-1] + (2 * codes.shape[-1],)).long()
        el = torch.tensor(E2M1_VALUES, dtype=torch.float64)[nib & 7] * (1.0 - 2.0 * (nib >> 3).double())
    D = el.shape[-1]
    if tuple(scales.shape) != tuple(el.shape[:-1]) + (D // 32,) or scales.dtype != torch.uint8:
        raise ValueError(f"mx_dequantize_host: uint8 scale bytes {list(el.shape[:-1]) + [D // 32]}, got {tuple(scales.shape)} {scales.dtype}")
    two = torch.pow(torch.tensor(2.0, dtype=torch.float64), scales.double() - 127.0)
    return (el.reshape(el.shape[:-1] + (D // 32, 32)) * two[..., None]).reshape(el.shape)


def mx_scores_host(codesA, scaleA, codesB, scaleB, maskA, maskB, wA, wB):
    """What valor_fine_fused_fwd_mx computes, in fp64 on the CPU: compute_fine_matrix_slice (pretrain.py:191-211) on the dequantised
    rows. codesA uint8 [NA, T, D] (MX e4m3), scaleA uint8 [NA, T, D / 32], codesB uint8 [NB, Nv, D / 2] (MX e2m1), scaleB uint8 [NB, Nv,
    D / 32], masks and SOFTMAXED token weights [NA, T] / [NB, Nv]. [NA, NB] fp64."""
    f64 = lambda t: t.detach().cpu().double()
    sim = torch.einsum("atd,bvd->abtv", mx_dequantize_host(codesA, scaleA, MX_E4M3), mx_dequantize_host(codesB, scaleB, MX_E2M1))
    x = sim * f64(maskA)[:, None, :, None] * f64(maskB)[None, :, None, :]
    return (torch.einsum("abt,at->ab", x.max(dim=3)[0], f64(wA)) + torch.einsum("abv,bv->ab", x.max(dim=2)[0], f64(wB))) / 2.0


def mx_quantize_rows(x, fmt):
    """valor_mx_quantize_rows on device bf16 / fp32 rows x [..., D] (D % 32 == 0; a 2-D x may be a column slice of a wider matrix):
    (uint8 codes [..., D] (MX_E4M3) or [..., D / 2] (MX_E2M1), dense; uint8 scale bytes [..., D / 32]). A non-finite value raises
    ValueError, as quantize_rows does."""
    _mx_format(fmt)
    K._check_gpu(x)
    if x.dtype not in (torch.bfloat16, torch.float32) or x.dim() < 1 or x.shape[-1] % 32 or x.shape[-1] == 0:
        raise ValueError(f"mx_quantize_rows: bf16 or fp32 rows of a multiple of 32 elements, got {tuple(x.shape)} {x.dtype}")
    cols = x.shape[-1]
    strided = x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= cols and (x.stride(0) * x.element_size()) % 16 == 0 and x.data_ptr() % 16 == 0
    if not strided:
        x = x.contiguous()
    if not bool(torch.isfinite(x).all()):
        raise ValueError("mx_quantize_rows: the rows hold a non-finite value")
    rows = x.numel() // cols
    codes = torch.empty(x.shape[:-1] + (cols if fmt == MX_E4M3 else cols // 2,), dtype=torch.uint8, device=x.device)
    scales = torch.empty(x.shape[:-1] + (cols // 32,), dtype=torch.uint8, device=x.device)
    lib.call("valor_mx_quantize_rows", K._stream(), 0 if x.dtype == torch.bfloat16 else 1, x.data_ptr(), x.stride(0) if strided else cols, rows,
             cols, fmt, codes.data_ptr(), scales.data_ptr())
    return codes, scales


def _scores_mx(qc, qs, bc, bs, maskA, maskB, wA, wB, out):
    """out [NA, nb] (dense fp32) = valor_fine_fused_fwd_mx on contiguous codes / scale bytes, the A rows in pieces under the kernel's byte limit"""
    NA, T, D = qc.shape
    nb, Nv = bc.shape[:2]
    st = K._stream()
    ra = max(1, min(NA, (E._FUSED_BYTES - 1) // (T * D)))
    for a0 in range(0, NA, ra):
        na = min(ra, NA - a0)
        lib.call("valor_fine_fused_fwd_mx", st, qc[a0:a0 + na].data_ptr(), qs[a0:a0 + na].data_ptr(), bc.data_ptr(), bs.data_ptr(),
                 maskA[a0:a0 + na].data_ptr(), maskB.data_ptr(), wA[a0:a0 + na].data_ptr(), wB.data_ptr(), out[a0:a0 + na].data_ptr(), na, nb, T, Nv, D)
    return out


# ------------------------------------------------------------------ pair scores: the law on the host (checks only) and the wrapper
EXACT_MODES = (None, "device", "host")
MAX_SHORTLIST = 256                   # valor_topk_rows selects at most 256 per row
# the default shortlist of a two-stage search is min(MAX_SHORTLIST, SHORTLIST_FACTOR * k). The 4 began as a starting point nobody had
# measured; DESIGN.md section 3.4 (profiles/search_rescore_bench.json) holds the measurement and says whether it moved.
SHORTLIST_FACTOR = 4
# an mxfp4 walk is coarser: on the bench geometry 4 k returned 0.984 - 1.0 of the exact top 10, 8 k all of it, at under 0.2 % more time at
# 10^6 clips and 64 queries (profiles/search_mx_bench.json)
SHORTLIST_FACTOR_MX = 8


def pair_scores_host(featA, maskA, wA, store, wstore, cand):
    """What valor_fine_score_pairs computes, in fp64 on the CPU: the law of fp8_scores_host on bf16-rounded features, for the pairs
    (query a, clip cand[a, c]) only, the clip mask all ones. featA [NA, T, D], maskA and SOFTMAXED wA [NA, T], store [NS, Nv, D], SOFTMAXED
    wstore [NS, Nv], cand int64 [NA, C]. A candidate outside [0, NS) scores -inf. [NA, C] fp64."""
    bf = lambda t: t.detach().cpu().to(torch.bfloat16).double()
    f64 = lambda t: t.detach().cpu().double()
    fa, fs, mA, wa, ws = bf(featA), bf(store), f64(maskA), f64(wA), f64(wstore)
    cand = cand.detach().cpu().long()
    NS = fs.shape[0]
    ok = (cand >= 0) & (cand < NS)
    safe = torch.where(ok, cand, torch.zeros_like(cand))
    out = torch.empty(cand.shape, dtype=torch.float64)
    for a in range(cand.shape[0]):
        x = torch.einsum("td,cvd->ctv", fa[a], fs[safe[a]]) * mA[a][None, :, None]
        out[a] = (x.max(dim=2)[0] @ wa[a] + (x.max(dim=1)[0] * ws[safe[a]]).sum(1)) / 2.0
    return torch.where(ok, out, torch.full_like(out, float("-inf")))


def score_pairs(ft, mask, wq, store, wstore, cand):
    """valor_fine_score_pairs: fp32 [NA, C] scores of the pairs (query a, clip cand[a, c]). ft bf16 [NA, T, D], mask and SOFTMAXED wq
    fp32 [NA, T], store bf16 [NS, Nv, D] and its SOFTMAXED weights fp32 [NS, Nv] (all contiguous, on the device), cand int64 [NA, C]
    with unit column stride. D % 64 == 0 and at most 64 tokens on either side; a candidate outside [0, NS) scores -inf."""
    K._check_gpu(ft, mask, wq, store, wstore, cand)
    if ft.dtype != torch.bfloat16 or store.dtype != torch.bfloat16 or ft.dim() != 3 or store.dim() != 3 or ft.shape[2] != store.shape[2]:
        raise ValueError(f"score_pairs: bf16 [NA, T, D] queries and a bf16 [NS, Nv, D] store, got {tuple(ft.shape)} {ft.dtype}, {tuple(store.shape)} {store.dtype}")
    NA, T, D = ft.shape
    NS, Nv = store.shape[:2]
    if D % 64 or D == 0 or not 1 <= T <= 64 or not 1 <= Nv <= 64:
        raise ValueError(f"score_pairs: D % 64 == 0 and 1 .. 64 tokens on either side (valor_fine_score_pairs has no fallback), got T={T}, Nv={Nv}, D={D}")
    for name, t, shape in (("mask", mask, (NA, T)), ("wq", wq, (NA, T)), ("wstore", wstore, (NS, Nv))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"score_pairs: {name}: a contiguous fp32 {list(shape)} tensor")
    if not ft.is_contiguous() or not store.is_contiguous():
        raise ValueError("score_pairs: contiguous features")
    if cand.dtype != torch.int64 or cand.dim() != 2 or cand.shape[0] != NA or (cand.shape[1] > 1 and cand.stride(1) != 1):
        raise ValueError(f"score_pairs: cand: an int64 [{NA}, C] tensor with unit column stride")
    C = cand.shape[1]
    out = torch.empty((NA, C), dtype=torch.float32, device=ft.device)
    if NA and C:
        lib.call("valor_fine_score_pairs", K._stream(), ft.data_ptr(), mask.data_ptr(), wq.data_ptr(), store.data_ptr(), wstore.data_ptr(), NS,
                 cand.data_ptr(), cand.stride(0) if NA > 1 else max(cand.stride(0), C), out.data_ptr(), C, NA, C, T, Nv, D)
    return out


# ------------------------------------------------------------------ pair alignments: the law on the host (checks only) and the wrapper
def credits_host(a2b, idx_a, b2a, idx_b, wA, wB):
    """The credit sequence of valor_fine_align_pairs on given maxima and arg-max bytes, in fp32 on the CPU, every step rounded on its
    own: termA = 0.5 * (wA * a2b); termB = wB != 0 ? 0.5 * (wB * b2a) : 0; credit_b[v] = termB[v], then + termA[t] for t ascending
    with idx_a[t] == v; credit_a[t] = termA[t], then + termB[v] for v ascending with idx_b[v] == t. a2b / idx_a [..., T], b2a / idx_b
    [..., Nv]; wA and wB broadcast against them. Returns (credit_a fp32 [..., T], credit_b fp32 [..., Nv])."""
    f32 = lambda t: torch.as_tensor(t).detach().cpu().float()
    a2b, b2a = f32(a2b), f32(b2a)
    ia, ib = torch.as_tensor(idx_a).detach().cpu().long(), torch.as_tensor(idx_b).detach().cpu().long()
    wA, wB = f32(wA).expand_as(a2b), f32(wB).expand_as(b2a)
    T, Nv = a2b.shape[-1], b2a.shape[-1]
    termA = 0.5 * (wA * a2b)
    termB = torch.where(wB != 0, 0.5 * (wB * b2a), torch.zeros_like(b2a))
    credit_a, credit_b = termA.clone(), termB.clone()
    slots_v, slots_t = torch.arange(Nv), torch.arange(T)
    for t in range(T):
        credit_b = torch.where(ia[..., t, None] == slots_v, credit_b + termA[..., t, None], credit_b)
    for v in range(Nv):
        credit_a = torch.where(ib[..., v, None] == slots_t, credit_a + termB[..., v, None], credit_a)
    return credit_a, credit_b


def align_pairs_host(featA, maskA, wA, store, wstore, cand, sim=False):
    """What valor_fine_align_pairs computes, on the CPU: for the pairs (query a, clip cand[a, c]) x = S * maskA in fp64 on the
    bf16-rounded features (the clip mask all ones), the maxima and FIRST arg maxima of either direction from it, the score as
    pair_scores_host, and the credits by credits_host on the fp32-rounded maxima. A candidate outside [0, NS): score -inf, index
    bytes 255, every other number 0. A dict: score fp64 [NA, C]; a2b fp64, idx_a uint8 [NA, C, T]; b2a fp64, idx_b uint8 [NA, C, Nv];
    credit_a fp32 [NA, C, T]; credit_b fp32 [NA, C, Nv]; sim fp64 [NA, C, T, Nv] or None."""
    bf = lambda t: t.detach().cpu().to(torch.bfloat16).double()
    f64 = lambda t: t.detach().cpu().double()
    fa, fs, mA, wa, ws = bf(featA), bf(store), f64(maskA), f64(wA), f64(wstore)
    cand = cand.detach().cpu().long()
    NA, C = cand.shape
    NS, Nv = fs.shape[:2]
    T = fa.shape[1]
    ok = (cand >= 0) & (cand < NS)
    safe = torch.where(ok, cand, torch.zeros_like(cand))
    x = torch.empty((NA, C, T, Nv), dtype=torch.float64)
    for a in range(NA):
        x[a] = torch.einsum("td,cvd->ctv", fa[a], fs[safe[a]]) * mA[a][None, :, None]
    xn = x.numpy()                                                       # numpy's argmax is the FIRST maximal index
    a2b, b2a = x.max(dim=3)[0], x.max(dim=2)[0]
    idx_a, idx_b = torch.from_numpy(xn.argmax(axis=3)), torch.from_numpy(xn.argmax(axis=2))
    wsel = ws[safe] if NS else torch.zeros((NA, C, Nv), dtype=torch.float64)
    score = ((a2b * wa[:, None, :]).sum(-1) + (b2a * wsel).sum(-1)) / 2.0
    live3, live4 = ok[:, :, None], ok[:, :, None, None]
    a2b, b2a = torch.where(live3, a2b, torch.zeros_like(a2b)), torch.where(live3, b2a, torch.zeros_like(b2a))
    idx_a = torch.where(live3, idx_a, torch.full_like(idx_a, 255)).to(torch.uint8)
    idx_b = torch.where(live3, idx_b, torch.full_like(idx_b, 255)).to(torch.uint8)
    credit_a, credit_b = credits_host(a2b, idx_a, b2a, idx_b, wa[:, None, :], torch.where(live3, wsel, torch.zeros_like(wsel)))
    return dict(score=torch.where(ok, score, torch.full_like(score, float("-inf"))), a2b=a2b, idx_a=idx_a, b2a=b2a, idx_b=idx_b,
                credit_a=credit_a, credit_b=credit_b, sim=torch.where(live4, x, torch.zeros_like(x)) if sim else None)


def align_pairs(ft, mask, wq, store, wstore, cand, sim=False):
    """valor_fine_align_pairs on the pairs (query a, clip cand[a, c]): a dict of device tensors score fp32 [NA, C]; a2b fp32, idx_a
    uint8 [NA, C, T]; b2a fp32, idx_b uint8 [NA, C, Nv]; credit_a fp32 [NA, C, T]; credit_b fp32 [NA, C, Nv]; sim fp32 [NA, C, T, Nv]
    (sim=True) or None. Arguments and coverage as score_pairs; a candidate outside [0, NS) gives -inf, 255 and zeros."""
    K._check_gpu(ft, mask, wq, store, wstore, cand)
    if ft.dtype != torch.bfloat16 or store.dtype != torch.bfloat16 or ft.dim() != 3 or store.dim() != 3 or ft.shape[2] != store.shape[2]:
        raise ValueError(f"align_pairs: bf16 [NA, T, D] queries and a bf16 [NS, Nv, D] store, got {tuple(ft.shape)} {ft.dtype}, {tuple(store.shape)} {store.dtype}")
    NA, T, D = ft.shape
    NS, Nv = store.shape[:2]
    if D % 64 or D == 0 or not 1 <= T <= 64 or not 1 <= Nv <= 64:
        raise ValueError(f"align_pairs: D % 64 == 0 and 1 .. 64 tokens on either side (valor_fine_align_pairs has no fallback), got T={T}, Nv={Nv}, D={D}")
    for name, t, shape in (("mask", mask, (NA, T)), ("wq", wq, (NA, T)), ("wstore", wstore, (NS, Nv))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"align_pairs: {name}: a contiguous fp32 {list(shape)} tensor")
    if not ft.is_contiguous() or not store.is_contiguous():
        raise ValueError("align_pairs: contiguous features")
    if cand.dtype != torch.int64 or cand.dim() != 2 or cand.shape[0] != NA or (cand.shape[1] > 1 and cand.stride(1) != 1):
        raise ValueError(f"align_pairs: cand: an int64 [{NA}, C] tensor with unit column stride")
    C = cand.shape[1]
    f32, u8 = dict(dtype=torch.float32, device=ft.device), dict(dtype=torch.uint8, device=ft.device)
    out = dict(score=torch.empty((NA, C), **f32), a2b=torch.empty((NA, C, T), **f32), idx_a=torch.empty((NA, C, T), **u8),
               b2a=torch.empty((NA, C, Nv), **f32), idx_b=torch.empty((NA, C, Nv), **u8), credit_a=torch.empty((NA, C, T), **f32),
               credit_b=torch.empty((NA, C, Nv), **f32), sim=torch.empty((NA, C, T, Nv), **f32) if sim else None)
    if NA and C:
        lib.call("valor_fine_align_pairs", K._stream(), ft.data_ptr(), mask.data_ptr(), wq.data_ptr(), store.data_ptr(), wstore.data_ptr(), NS,
                 cand.data_ptr(), cand.stride(0) if NA > 1 else max(cand.stride(0), C), NA, C, T, Nv, D,
                 *[None if out[n] is None else out[n].data_ptr() for n in ("score", "a2b", "idx_a", "b2a", "idx_b", "credit_a", "credit_b", "sim")])
    return out


MODALITIES = ("video", "audio")


def _check_layout(layout, tokens):
    """one part's token layout as a list of (modality, count) whose counts cover the part's tokens, or ValueError"""
    try:
        layout = [(str(m), int(n)) for m, n in layout]
    except (TypeError, ValueError):
        raise ValueError(f"token_layout: per part a list of (modality, count), got {layout!r}")
    if any(m not in MODALITIES or n < 1 for m, n in layout) or sum(n for _, n in layout) != tokens:
        raise ValueError(f"token_layout {layout}: modalities from {MODALITIES}, counts >= 1 that add up to the part's {tokens} tokens")
    return layout


class AlignmentPart:
    """the alignment of one bank part, device tensors: score fp32 [NQ, C]; text_max fp32 / text_best uint8 [NQ, C, T] (every query token's
    best clip token: value, slot); clip_max / clip_best [NQ, C, Nv] (every clip token's best query token); text_credit [NQ, C, T] and
    clip_credit [NQ, C, Nv] (the part's score split over the tokens of either side); sim fp32 [NQ, C, T, Nv] or None; layout: the part's
    [(modality, count), ...] or None."""

    def __init__(self, out, layout):
        self.score, self.text_max, self.text_best, self.clip_max, self.clip_best = out["score"], out["a2b"], out["idx_a"], out["b2a"], out["idx_b"]
        self.text_credit, self.clip_credit, self.sim, self.layout = out["credit_a"], out["credit_b"], out["sim"], layout


class Alignment:
    """indices int64 [NQ, C] (bank indices; -1 = an empty slot: 255 / 0 in every part) and parts: one AlignmentPart, or two (video,
    audio) under late fusion, each with its part's stored weights."""

    def __init__(self, indices, parts):
        self.indices, self.parts = indices, list(parts)

    def _layouts(self):
        if any(p.layout is None for p in self.parts):
            raise ValueError("the index has no token_layout (a fused 'tva' bank built from features: pass from_features(..., token_layout=))")
        return [p.layout for p in self.parts]

    def clip_credit_by_modality(self):
        """{"video": [NQ, C], "audio": [NQ, C]} fp32 on the device: the clip credits of every layout entry summed, added over the parts
        (a modality the bank does not hold: zeros). Nothing is read back."""
        out = {m: torch.zeros(self.indices.shape, dtype=torch.float32, device=self.indices.device) for m in MODALITIES}
        for part, layout in zip(self.parts, self._layouts()):
            v0 = 0
            for m, n in layout:
                out[m] = out[m] + part.clip_credit[:, :, v0:v0 + n].sum(-1)
                v0 += n
        return out

    def best_clip_token(self):
        """(part, modality index, token index within the modality), int64 [NQ, C] each, on the device: the clip token of largest credit
        over all parts, the lowest (part, token) among equals (an equality mask and a min over positions: no arg max whose tie rule is
        unspecified); the modality index counts the entries of the part's layout. An empty slot holds -1."""
        layouts = self._layouts()
        dev = self.indices.device
        credit = torch.cat([p.clip_credit for p in self.parts], dim=-1)
        n = credit.shape[-1]
        pos = torch.arange(n, dtype=torch.int64, device=dev)
        first = torch.where(credit == credit.amax(-1, keepdim=True), pos, torch.full_like(pos, n)).amin(-1).clamp(max=n - 1)
        table = [(pi, mi, j) for pi, layout in enumerate(layouts) for mi, (_, cnt) in enumerate(layout) for j in range(cnt)]
        table = torch.tensor(table, dtype=torch.int64, device=dev)
        got = table[first]
        got = torch.where((self.indices >= 0)[..., None], got, torch.full_like(got, -1))
        return got[..., 0], got[..., 1], got[..., 2]


def within_prepare(cand, NB):
    """The candidate rows of a subset search, made ready for the selection (torch ops: the device path and the host plan share them):
    every row sorted ascending, repeated entries and entries outside [0, NB) turned into -1. A position then stands for one clip, and
    position order is bank index order, so valor_topk_rows' tie rule (position ascending) is the search's (bank index ascending)."""
    srt = torch.sort(cand, dim=1)[0]
    dup = torch.zeros_like(srt, dtype=torch.bool)
    dup[:, 1:] = srt[:, 1:] == srt[:, :-1]
    return torch.where(dup | (srt < 0) | (srt >= NB), torch.full_like(srt, -1), srt)


def within_finish(top_val, top_pos, srt):
    """positions of the selection -> bank indices; a slot that selected nothing, or a -1 entry, is -inf / -1"""
    idx = torch.where(top_pos >= 0, srt.gather(1, top_pos.clamp(min=0)), torch.full_like(top_pos, -1))
    return torch.where(idx >= 0, top_val, torch.full_like(top_val, float("-inf"))), idx


def within_host(score, cand, k):
    """The plan of search(within=) on the host, on a full score matrix [NQ, NB] (checks only): sort ascending, de-duplicate, gather the
    pair scores, topk_host, map back. (val fp32 [NQ, k], idx int64 [NQ, k])."""
    score = score.detach().float().cpu()
    srt = within_prepare(cand.detach().cpu().long(), score.shape[1])
    pair = torch.where(srt >= 0, score.gather(1, srt.clamp(min=0)), torch.full(srt.shape, float("-inf")))
    return within_finish(*topk_host(pair, k), srt)


class SearchResult:
    """scores fp32 [NQ, k] and indices int64 [NQ, k] on the device (-inf / -1 where the bank has fewer than k clips); `.ids` reads the
    indices back and maps them to the bank's clip ids (None for -1). `alignment`: the Alignment of exactly these indices after
    search(..., explain=True), None otherwise. `groups`: the group id of every returned clip, int32 [NQ, k] on the device (-1: no
    clip, or a clip without a group); `.group_labels` reads them back and maps them to the index's labels (None for -1). Iterating
    gives (ids, scores, indices)."""

    def __init__(self, scores, indices, bank_ids, alignment=None, groups=None, labels=()):
        self.scores, self.indices, self._bank_ids, self._ids = scores, indices, bank_ids, None
        self.alignment = alignment
        self._groups, self._labels, self._group_labels = groups, labels, None

    @property
    def ids(self):
        if self._ids is None:
            self._ids = [[self._bank_ids[j] if j >= 0 else None for j in row] for row in self.indices.cpu().tolist()]
        return self._ids

    @property
    def groups(self):
        if self._groups is None:                                         # an index without groups
            self._groups = torch.full(self.indices.shape, -1, dtype=torch.int32, device=self.indices.device)
        return self._groups

    @property
    def group_labels(self):
        if self._group_labels is None:
            self._group_labels = [[self._labels[g] if g >= 0 else None for g in row] for row in self.groups.cpu().tolist()]
        return self._group_labels

    def __iter__(self):
        return iter((self.ids, self.scores, self.indices))


def _pinned_empty(shape, dtype):
    """host memory the device can copy from without a staging step; plain host memory where there is no GPU (a CPU index is kept, saved
    and loaded, never searched)"""
    return torch.empty(shape, dtype=dtype, pin_memory=torch.cuda.is_available())


class _Bank:
    """one growing tensor [capacity, ...]; the first n rows are filled. On the device of its first rows, or (pin) in pinned host memory."""

    def __init__(self, first, pin=False):
        self.pin = pin
        if pin:
            self.data = _pinned_empty(tuple(first.shape), first.dtype)
            self.data.copy_(first)
        else:
            self.data = first.contiguous()
        self.n = first.shape[0]

    def append(self, rows):
        if rows.shape[1:] != self.data.shape[1:] or rows.dtype != self.data.dtype:
            raise ValueError(f"bank rows {tuple(rows.shape[1:])} {rows.dtype} against {tuple(self.data.shape[1:])} {self.data.dtype}")
        need = self.n + rows.shape[0]
        if need > self.data.shape[0]:                                  # doubling: add() is amortised
            shape = (max(need, 2 * self.data.shape[0]),) + tuple(self.data.shape[1:])
            grown = _pinned_empty(shape, self.data.dtype) if self.pin else torch.empty(shape, dtype=self.data.dtype, device=self.data.device)
            grown[:self.n] = self.data[:self.n]
            self.data = grown
        self.data[self.n:need] = rows.to(self.data.device)
        self.n = need

    def view(self):
        return self.data[:self.n]


def _softmax_ones_mask(raw):
    """valor_fine_weight_softmax over an all-ones mask, as validate_ret applies it to a clip's token weights"""
    K._check_gpu(raw)
    raw = raw.float().contiguous()
    out = torch.empty_like(raw)
    lib.call("valor_fine_weight_softmax", K._stream(), raw.data_ptr(), torch.ones_like(raw).data_ptr(), out.data_ptr(), raw.shape[0], raw.shape[1])
    return out


class RetrievalIndex:
    """A clip bank on the device for one retrieval group ('tv', 'tva', 'ta'). parts: one (features, weights) pair, or two under
    late_fusion 'tva' (video, audio: their scores are added). weights are the softmaxed token weights of a fine bank, None for coarse.
    bank_dtype "fp8" (fine banks): the parts are stored as e4m3 codes and row scales. `feats` are then bf16 / fp32 device features,
    quantised here, or -- with `scales` (one fp32 [clips, tokens] tensor per part) and `dtype` (the feature dtype the codes were made
    from) -- the uint8 codes themselves, on any device.
    bank_dtype "mxfp4" (fine banks): the parts are stored as MX e2m1 codes [clips, tokens, D / 2] and E8M0 block scale bytes; given as
    codes, `scales` are the uint8 [clips, tokens, D / 32] scale bytes. Everything an fp8 bank has, it has.
    exact "device" / "host" (fp8 and mxfp4 banks of bf16 features): the features the codes were made from are kept as well, on the bank's device
    or in pinned host memory (the device then holds only the codes); search() re-scores its shortlist on them. With codes given,
    `exact_feats` are those features, one bf16 [clips, tokens, D] tensor per part."""

    def __init__(self, group, contra_type, late_fusion, feats, weights, ids, bank_dtype=None, *, scales=None, dtype=None, exact=None,
                 exact_feats=None, token_layout=None):
        if group not in GROUPS:
            raise ValueError(f"group {group!r}: one of {GROUPS} (the va / vta / atv directions are not searchable)")
        if contra_type not in ("fine", "coarse"):
            raise ValueError(f"contra_type {contra_type!r}")
        if bank_dtype not in BANK_DTYPES:
            raise ValueError(f"bank_dtype {bank_dtype!r}: one of {BANK_DTYPES}")
        if bank_dtype == "fp8" and contra_type != "fine":
            raise ValueError("bank_dtype='fp8': only fine banks are covered (a coarse bank needs an fp8 GEMM)")
        if bank_dtype == "mxfp4" and contra_type != "fine":
            raise ValueError("bank_dtype='mxfp4': only fine banks are covered (a coarse bank needs a block-scaled GEMM)")
        if exact not in EXACT_MODES:
            raise ValueError(f"exact {exact!r}: one of {EXACT_MODES}")
        if exact is not None and bank_dtype not in _QUANTISED:
            raise ValueError("exact=: only an fp8 bank keeps a second, exact store (a bf16 bank is its own: rescore() reads it directly)")
        self.group, self.contra_type, self.late_fusion, self.bank_dtype = group, contra_type, bool(late_fusion), bank_dtype
        self.exact = exact
        nparts = 2 if (self.late_fusion and group == "tva") else 1
        if len(feats) != nparts or len(weights) != nparts:
            raise ValueError(f"group {group!r}, late_fusion={self.late_fusion}: {nparts} feature bank(s), got {len(feats)}")
        dims = 3 if contra_type == "fine" else 2
        for f, w in zip(feats, weights):
            if f.dim() != dims or f.shape[0] != len(ids) or f.shape[-1] != feats[0].shape[-1] or f.dtype != feats[0].dtype:
                raise ValueError(f"a {contra_type} bank holds [{len(ids)} clips, {'tokens, ' if dims == 3 else ''}D] features, got {tuple(f.shape)}")
            if (w is None) != (contra_type == "coarse") or (w is not None and (tuple(w.shape) != tuple(f.shape[:2]) or w.dtype != torch.float32)):
                raise ValueError("a fine bank carries fp32 token weights [clips, tokens], a coarse bank none")
        self._scales = None
        self._exact, self._stage = None, {}
        if bank_dtype == "fp8":
            for f in feats:
                if f.shape[-1] % 128 or f.shape[1] > 64 or f.shape[1] < 1:
                    raise ValueError(f"bank_dtype='fp8': D % 128 == 0 and 1 .. 64 tokens per clip (valor_fine_fused_fwd_fp8 has no GEMM "
                                     f"fallback), got {tuple(f.shape)}")
            if scales is None:
                self._dtype = feats[0].dtype
                exact_feats = feats if exact is not None else None
                feats, scales = zip(*[quantize_rows(f) for f in feats])
            else:
                if (feats[0].dtype != torch.uint8 or dtype not in (torch.bfloat16, torch.float32) or len(scales) != nparts
                        or any(tuple(s.shape) != tuple(f.shape[:2]) or s.dtype != torch.float32 for f, s in zip(feats, scales))):
                    raise ValueError("an fp8 bank given as codes: uint8 [clips, tokens, D], fp32 scales [clips, tokens], dtype bf16 / fp32")
                self._dtype = dtype
            if exact is not None:
                if (self._dtype != torch.bfloat16 or exact_feats is None or len(exact_feats) != nparts
                        or any(e.dtype != torch.bfloat16 or tuple(e.shape) != tuple(f.shape) for e, f in zip(exact_feats, feats))):
                    raise ValueError("exact=: the store holds the bf16 features the codes were made from, one [clips, tokens, D] tensor per "
                                     "part (valor_fine_score_pairs scores bf16 only)")
                # "device": a copy of its own (the caller's tensor is not aliased, as the codes are not); "host": pinned, growing
                self._exact = [_Bank(e, pin=True) if exact == "host" else _Bank(e.to(feats[0].device).clone()) for e in exact_feats]
            self._scales = [_Bank(s) for s in scales]
        if bank_dtype == "mxfp4":
            # given as features: [clips, tokens, D] bf16 / fp32, quantised here; given as codes (`scales`): uint8 [clips, tokens, D / 2]
            # with uint8 scale bytes [clips, tokens, D / 32]. D is the feature dimension either way.
            given = scales is not None
            for f in feats:
                D = f.shape[-1] * (2 if given else 1)
                if D % 128 or D == 0 or f.shape[1] > 64 or f.shape[1] < 1:
                    raise ValueError(f"bank_dtype='mxfp4': D % 128 == 0 and 1 .. 64 tokens per clip (valor_fine_fused_fwd_mx has no GEMM "
                                     f"fallback), got {tuple(f.shape[:2]) + (D,)}")
            if not given:
                self._dtype = feats[0].dtype
                exact_feats = feats if exact is not None else None
                feats, scales = zip(*[mx_quantize_rows(f, MX_E2M1) for f in feats])
            else:
                if (feats[0].dtype != torch.uint8 or dtype not in (torch.bfloat16, torch.float32) or len(scales) != nparts
                        or any(tuple(s.shape) != tuple(f.shape[:2]) + (f.shape[2] // 16,) or s.dtype != torch.uint8 for f, s in zip(feats, scales))):
                    raise ValueError("an mxfp4 bank given as codes: uint8 [clips, tokens, D / 2], uint8 scale bytes [clips, tokens, D / 32], "
                                     "dtype bf16 / fp32")
                self._dtype = dtype
            if exact is not None:
                if (self._dtype != torch.bfloat16 or exact_feats is None or len(exact_feats) != nparts
                        or any(e.dtype != torch.bfloat16 or tuple(e.shape) != tuple(f.shape[:2]) + (2 * f.shape[2],) for e, f in zip(exact_feats, feats))):
                    raise ValueError("exact=: the store holds the bf16 features the codes were made from, one [clips, tokens, D] tensor per "
                                     "part (valor_fine_score_pairs scores bf16 only)")
                self._exact = [_Bank(e, pin=True) if exact == "host" else _Bank(e.to(feats[0].device).clone()) for e in exact_feats]
            self._scales = [_Bank(s) for s in scales]
        self._feats = [_Bank(f) for f in feats]
        self._weights = [None if w is None else _Bank(w) for w in weights]
        self.ids = list(ids)
        self.token_layout = self._token_layout(token_layout)
        # only a fused 'tva' bank's layout cannot be inferred from the group and the token counts: it alone is saved and handed on
        self._layout_saved = self.token_layout is not None and group == "tva" and nparts == 1
        # the selection's bookkeeping: nothing until remove() / groups= ask for it, and an index without it calls valor_topk_rows
        self._alive, self._removed = None, 0                             # device bool [capacity]: False = removed
        self._groups, self.group_labels, self._label_id = None, [], {}   # device int32 [capacity] (-1: none); id -> label; label -> id
        self._positions = None                                           # clip id -> positions, built by remove(ids=)

    # ------------------------------------------------------------------ removal and groups
    @property
    def live(self):
        """the number of clips not removed (len() stays the number of positions)"""
        return len(self.ids) - self._removed

    @property
    def alive(self):
        """device bool [NB]: False for a removed clip; None while nothing was removed"""
        return None if self._alive is None else self._alive.view()

    @property
    def groups(self):
        """device int32 [NB]: every clip's group id into group_labels, -1 for a clip of no group; None for an index without groups"""
        return None if self._groups is None else self._groups.view()

    def _append_groups(self, n, labels, before=None):
        """the group column of n rows about to be appended to a bank of `before` rows (default: its present length): labels one
        hashable per row (None: no group) or None altogether; the label table grows by the labels not seen before"""
        if labels is None:
            if self._groups is not None:
                self._groups.append(torch.full((n,), -1, dtype=torch.int32, device=self.device))
            return
        labels = list(labels)
        if len(labels) != n:
            raise ValueError(f"groups: one label per row ({n}), got {len(labels)}")
        gid = []
        for lab in labels:
            if lab is not None and lab not in self._label_id:
                self._label_id[lab] = len(self.group_labels)
                self.group_labels.append(lab)
            gid.append(-1 if lab is None else self._label_id[lab])
        rows = torch.tensor(gid, dtype=torch.int32).to(self.device)
        if self._groups is None:                                         # the rows added before carried no label
            before = len(self.ids) if before is None else before
            self._groups = _Bank(torch.cat((torch.full((before,), -1, dtype=torch.int32, device=self.device), rows)))
        else:
            self._groups.append(rows)

    def remove(self, ids=None, indices=None):
        """Tombstone clips, named by clip id (every position holding the id) or by bank index: they are never returned by search() again,
        on any path; an entry of a within= list that names one counts as -1. Positions keep their meaning (compact() reclaims the
        rows), rescore() / explain() on explicit indices still read them. An id the bank does not hold raises KeyError, an index outside
        it IndexError, before anything changes. Returns the number of clips newly removed (one read-back)."""
        if (ids is None) == (indices is None):
            raise ValueError("remove: ids= or indices=, one of them")
        NB = len(self.ids)
        if ids is not None:
            if self._positions is None:
                self._positions = {}
                for j, cid in enumerate(self.ids):
                    self._positions.setdefault(cid, []).append(j)
            pos = []
            for cid in ids:
                if cid not in self._positions:
                    raise KeyError(f"remove: the bank holds no clip of id {cid!r}")
                pos += self._positions[cid]
        else:
            pos = [int(j) for j in (indices.tolist() if torch.is_tensor(indices) else indices)]
            if any(j < 0 or j >= NB for j in pos):
                raise IndexError(f"remove: bank indices lie in [0, {NB})")
        if not pos:
            return 0
        if self._alive is None:
            self._alive = _Bank(torch.ones((NB,), dtype=torch.bool, device=self.device))
        pos = torch.unique(torch.tensor(pos, dtype=torch.int64)).to(self.device)
        alive = self._alive.view()
        newly = int(alive[pos].sum())
        alive[pos] = False
        self._removed += newly
        return newly

    def compact(self):
        """Rewrite every store without the removed rows (features or codes, scales, weights, the exact store, ids, groups; the label
        table keeps the labels that still have a clip, in the order of their first one). Afterwards the index is what from_features /
        build on the surviving rows would have made. Returns the old -> new index map, int64 [old NB] on the device, -1 for a removed
        row."""
        NB = len(self.ids)
        dev = self.device
        if self._alive is None or not self._removed:
            self._alive, self._removed = None, 0
            return torch.arange(NB, dtype=torch.int64, device=dev)
        stay = torch.nonzero(self._alive.view()).view(-1)
        remap = torch.full((NB,), -1, dtype=torch.int64, device=dev)
        remap[stay] = torch.arange(stay.numel(), dtype=torch.int64, device=dev)
        stay_host = stay.cpu()
        shrink = lambda bank: None if bank is None else _Bank(bank.view().index_select(0, stay_host if bank.pin else stay), pin=bank.pin)
        self._feats = [shrink(b) for b in self._feats]
        self._weights = [shrink(b) for b in self._weights]
        if self._scales is not None:
            self._scales = [shrink(b) for b in self._scales]
        if self._exact is not None:
            self._exact = [shrink(b) for b in self._exact]
        self.ids = [self.ids[j] for j in stay_host.tolist()]
        if self._groups is not None:
            old, labels = self._groups.view().index_select(0, stay).cpu().tolist(), self.group_labels
            self._groups, self.group_labels, self._label_id = None, [], {}
            self._append_groups(len(old), [labels[g] if g >= 0 else None for g in old], before=0)
        self._alive, self._removed, self._positions, self._stage = None, 0, None, {}
        return remap

    def update(self, ids, feats, weights, groups=None, token_layout=None):
        """Replace clips: remove(ids=ids), then add_features(feats, weights, ids, ...). The new rows take new positions at the end; the
        old ones stay tombstoned until compact(). If the new rows are refused (a non-finite row of a quantised bank, another token
        count or layout, a wrong number of labels) the removal is undone and the error raised: the index is what it was. Returns the
        number of clips removed."""
        ids = list(ids)
        had = self._alive is not None
        before = self._alive.view().clone() if had else None
        removed = self.remove(ids=ids)
        try:
            self.add_features(feats, weights, ids, token_layout=token_layout, groups=groups)
        except Exception:
            if had:
                self._alive.view().copy_(before)
            else:
                self._alive = None
            self._removed -= removed
            raise
        return removed

    def _token_layout(self, given):
        """per part a list of (modality, count) over the clip's token axis, or None (a coarse bank; a fused 'tva' bank nobody described).
        'tv', 'ta' and the two parts of a late-fusion bank hold one modality each: inferred from the token count."""
        if self.contra_type != "fine":
            if given is not None:
                raise ValueError("token_layout: a coarse bank has no tokens")
            return None
        tokens = [int(b.data.shape[1]) for b in self._feats]
        inferred = {"tv": [[("video", tokens[0])]], "ta": [[("audio", tokens[0])]]}.get(self.group)
        if self.group == "tva" and len(tokens) == 2:
            inferred = [[("video", tokens[0])], [("audio", tokens[1])]]
        if given is None:
            return inferred
        given = list(given)
        if len(given) != len(tokens):
            raise ValueError(f"token_layout: one list of (modality, count) per bank part ({len(tokens)}), got {given!r}")
        given = [_check_layout(l, n) for l, n in zip(given, tokens)]
        if inferred is not None and given != inferred:
            raise ValueError(f"token_layout {given}: a {self.group!r} bank{' under late fusion' if len(tokens) == 2 else ''} holds {inferred}")
        return given

    # ------------------------------------------------------------------ description
    def __len__(self):
        return len(self.ids)

    @property
    def device(self):
        return self._feats[0].data.device

    @property
    def dtype(self):
        """the feature dtype the index was built from (an fp8 bank: what its codes were quantised from, and what queries may be)"""
        return self._dtype if self.bank_dtype in _QUANTISED else self._feats[0].data.dtype

    @property
    def dim(self):
        """the feature dimension D (an mxfp4 bank's code rows hold D / 2 bytes)"""
        return int(self._feats[0].data.shape[-1]) * (2 if self.bank_dtype == "mxfp4" else 1)

    @property
    def feats(self):
        return [b.view() for b in self._feats]

    @property
    def weights(self):
        return [None if b is None else b.view() for b in self._weights]

    @property
    def scales(self):
        """an fp8 bank's fp32 row scales [NB, Nv] per part, an mxfp4 bank's uint8 E8M0 block scale bytes [NB, Nv, D / 32] (`feats` are
        then the uint8 codes); None otherwise"""
        return None if self._scales is None else [b.view() for b in self._scales]

    @property
    def exact_feats(self):
        """the exact store of an fp8 bank: bf16 [NB, Nv, D] per part, on the device or in pinned host memory; None without one"""
        return None if self._exact is None else [b.view() for b in self._exact]

    def bank_bytes(self):
        """device bytes of the filled rows: features or codes, scales, token weights, and an exact store kept on the device"""
        banks = self._feats + [b for b in self._weights if b is not None] + (self._scales or [])
        if self.exact == "device":
            banks = banks + self._exact
        return sum(b.view().numel() * b.data.element_size() for b in banks)

    @property
    def unit_text_weights(self):
        """late-fusion fine scores use unit token weights on both sides (test.py:571-579)"""
        return self.contra_type == "fine" and len(self._feats) == 2

    def fingerprint(self):
        fp = {"group": self.group, "contra_type": self.contra_type, "late_fusion": self.late_fusion, "D": self.dim,
              "tokens": [int(b.data.shape[1]) if self.contra_type == "fine" else 1 for b in self._feats], "dtype": str(self.dtype)}
        if self.bank_dtype == "fp8":
            fp["bank_dtype"] = "fp8_e4m3"
        if self.bank_dtype == "mxfp4":
            fp["bank_dtype"] = "mxfp4_e2m1"
        if self.exact is not None:
            fp["exact"] = self.exact
        return fp

    def _check_model(self, model):
        sp = model.spec
        if sp.contra_type != self.contra_type or bool(sp.late_fusion) != self.late_fusion:
            raise ValueError(f"the index was built for contra_type={self.contra_type!r}, late_fusion={self.late_fusion}; the model has "
                             f"contra_type={sp.contra_type!r}, late_fusion={bool(sp.late_fusion)}")

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_features(cls, feats, weights=None, ids=None, *, group="tv", contra_type="fine", late_fusion=False, weights_softmaxed=False,
                      bank_dtype=None, exact=None, token_layout=None, groups=None):
        """An index over given tensors (device tensors; a CPU index can be saved and loaded but not searched). feats: [NB, Nv, D] (fine)
        or [NB, D] (coarse), or a (video, audio) pair for late_fusion 'tva'. weights (fine, one parts): the RAW token weights [NB, Nv],
        softmaxed here as validate_ret does; None = unit weights, which is what late_fusion always uses. weights_softmaxed: `weights`
        (one tensor per part) already are the softmaxed values. bank_dtype "fp8": the features are quantised on the device and dropped,
        unless exact "device" / "host" keeps them for the two-stage search. token_layout: per part a list of (modality, count) along the
        clip's token axis, e.g. [[("video", 8), ("audio", 2)]] for a fused 'tva' bank (one part: the list itself will do); 'tv', 'ta' and
        late-fusion banks infer theirs, a fused 'tva' bank without one has None (Alignment's per-modality methods then refuse).
        groups: one hashable label per clip (None: no group), e.g. the video a segment was cut from: search(collapse=True) returns
        one clip per label."""
        if token_layout and isinstance(token_layout[0], (list, tuple)) and token_layout[0] and isinstance(token_layout[0][0], str):
            token_layout = [token_layout]                                # one part given as the list itself
        if bank_dtype == "fp8" and contra_type != "fine":
            raise ValueError("bank_dtype='fp8': only fine banks are covered (a coarse bank needs an fp8 GEMM)")
        if bank_dtype == "mxfp4" and contra_type != "fine":
            raise ValueError("bank_dtype='mxfp4': only fine banks are covered (a coarse bank needs a block-scaled GEMM)")
        if group not in GROUPS:
            raise ValueError(f"group {group!r}: one of {GROUPS} (the va / vta / atv directions are not searchable)")
        feats = list(feats) if isinstance(feats, (list, tuple)) else [feats]
        if contra_type == "coarse":
            ws = [None] * len(feats)
        elif weights_softmaxed:
            ws = [w.float() for w in (weights if isinstance(weights, (list, tuple)) else [weights])]
        else:
            raw = list(weights) if isinstance(weights, (list, tuple)) else [weights] * len(feats)
            if late_fusion and group == "tva" and any(w is not None for w in raw):
                raise ValueError("late_fusion scores use unit token weights: pass none")
            ws = [_softmax_ones_mask(torch.ones(f.shape[:2], dtype=torch.float32, device=f.device) if w is None else w) for f, w in zip(feats, raw)]
        ids = list(range(feats[0].shape[0])) if ids is None else list(ids)
        index = cls(group, contra_type, late_fusion, feats, ws, ids, bank_dtype, exact=exact, token_layout=token_layout)
        index._append_groups(len(ids), groups, before=0)
        return index

    def quantize(self, exact=None, bank_dtype="fp8"):
        """A new fp8 (or, bank_dtype="mxfp4", MXFP4) index over this fine bf16 / fp32 bank, quantised on the device; this index is
        untouched. exact "device" / "host": the new index keeps a copy of the bf16 features beside the codes."""
        if self.bank_dtype is not None:
            raise ValueError("the bank is quantised already")
        if bank_dtype not in _QUANTISED:
            raise ValueError(f"quantize: bank_dtype {bank_dtype!r}: one of {_QUANTISED}")
        index = RetrievalIndex(self.group, self.contra_type, self.late_fusion, self.feats, [None if w is None else w.clone() for w in self.weights],
                               self.ids, bank_dtype, exact=exact, token_layout=self.token_layout)
        index._copy_selection(self.alive, self.groups, self.group_labels)
        return index

    @staticmethod
    def encode_gallery(model, batch, group):
        """The bank rows of one gallery batch: the encoders named by the group's letters run with the text side off (the letters of a
        'ret%..' group list choose the encoders; compute_loss=False returns feat_v / feat_a). Returns (feats, softmaxed weights)."""
        return RetrievalIndex._encode_gallery(model, batch, group)[:2]

    @staticmethod
    def _encode_gallery(model, batch, group):
        """encode_gallery and the rows' token layout (None for coarse rows): (feats, softmaxed weights, layout)"""
        if group not in GROUPS:
            raise ValueError(f"group {group!r}: one of {GROUPS}")
        P, sp = model.P, model.spec
        ev = model({k: v for k, v in batch.items() if k != "txt_tokens"}, task="ret%" + group.replace("t", ""), compute_loss=False)
        fv, fa = ev.get("feat_v"), ev.get("feat_a")
        late = bool(sp.late_fusion) and group == "tva"
        if sp.contra_type == "coarse":
            if group == "tva" and not late:
                feats = [ops.l2_normalize(ops.linear(torch.cat((fv, fa), dim=-1), P["va_fusion.weight"], P["va_fusion.bias"]))]
            else:
                feats = [f for f, c in ((fv, "v"), (fa, "a")) if c in group]
            return [f.detach().contiguous() for f in feats], [None] * len(feats), None
        named = [(n, f) for n, f, c in (("video", fv, "v"), ("audio", fa, "a")) if c in group]
        if late:
            feats = [f for _, f in named]
            return ([f.detach().contiguous() for f in feats], [_softmax_ones_mask(torch.ones(f.shape[:2], dtype=torch.float32, device=f.device)) for f in feats],
                    [[(n, int(f.shape[1]))] for n, f in named])
        feat = torch.cat([f for _, f in named], dim=1).detach().contiguous()
        raw = torch.cat([E._fine_weights(model, n, f) for n, f in named], dim=1)
        return [feat], [_softmax_ones_mask(raw)], [[(n, int(f.shape[1])) for n, f in named]]      # the concatenation order

    @classmethod
    @torch.no_grad()
    def build(cls, model, loader, group, bank_dtype=None, exact=None, group_key=None):
        """Encode every batch of `loader` (valor_collate batches with 'ids') once and keep the bank on the model's device
        (bank_dtype "fp8" / "mxfp4": as e4m3 / MX e2m1 codes, each batch quantised as it arrives; exact: the bf16 rows are kept too).
        group_key: the batch key that holds one group label per clip (e.g. the video a segment was cut from), or a callable
        batch -> labels."""
        labels = lambda batch: None if group_key is None else (group_key(batch) if callable(group_key) else batch[group_key])
        index = None
        model.eval()
        for batch in loader:
            if index is None:
                feats, ws, layout = cls._encode_gallery(model, batch, group)
                index = cls(group, model.spec.contra_type, bool(model.spec.late_fusion), feats, ws, list(batch["ids"]), bank_dtype, exact=exact,
                            token_layout=layout)
                index._append_groups(len(index), labels(batch), before=0)
            else:
                index.add(model, batch, groups=labels(batch))
        if index is None:
            raise ValueError("RetrievalIndex.build: the loader is empty")
        return index

    @torch.no_grad()
    def add(self, model, batch, groups=None):
        """Extend the bank in place by one gallery batch; earlier indices keep their meaning. groups: one label per clip, or None."""
        self._check_model(model)
        model.eval()
        feats, ws, layout = self._encode_gallery(model, batch, self.group)
        self.add_features(feats, ws, batch["ids"], token_layout=layout, groups=groups)

    def add_features(self, feats, weights, ids, token_layout=None, groups=None):
        """add() on encoded rows: one tensor per part, weights already softmaxed (None for coarse). An fp8 bank takes bf16 / fp32
        features and quantises them first; a non-finite row raises ValueError before anything is appended. token_layout: the rows'
        own layout, if the caller knows it; it must be the bank's (rows of another layout, or of another token count, are refused).
        groups: one hashable label per row (None: no group); rows added without one belong to no group."""
        ids = list(ids)
        if len(feats) != len(self._feats) or any(f.shape[0] != len(ids) for f in feats):
            raise ValueError("one feature tensor per bank part, one row per id")
        groups = None if groups is None else list(groups)
        if groups is not None and len(groups) != len(ids):
            raise ValueError(f"groups: one label per row ({len(ids)})")
        if self.contra_type == "fine":
            for bank, f in zip(self._feats, feats):
                if f.dim() != 3 or f.shape[1] != bank.data.shape[1]:
                    raise ValueError(f"rows of {tuple(f.shape[1:])} against a bank part of {int(bank.data.shape[1])} tokens per clip ({self.token_layout})")
            if token_layout is not None:
                rows = [_check_layout(l, int(f.shape[1])) for l, f in zip(token_layout, feats)]
                if self.token_layout is not None and rows != self.token_layout:
                    raise ValueError(f"rows of token_layout {rows} against the bank's {self.token_layout}")
        if self.bank_dtype == "fp8":
            for bank, f in zip(self._feats, feats):
                if f.shape[1:] != bank.data.shape[1:]:
                    raise ValueError(f"bank rows {tuple(f.shape[1:])} against {tuple(bank.data.shape[1:])}")
                if self._exact is not None and f.dtype != torch.bfloat16:
                    raise ValueError("an index with an exact store takes bf16 rows")
            rows = feats
            feats, scales = zip(*[quantize_rows(f) for f in feats])
            if self._exact is not None:                                  # after the quantiser: it refuses non-finite rows
                for bank, f in zip(self._exact, rows):
                    bank.append(f)
            for bank, s in zip(self._scales, scales):
                bank.append(s)
        if self.bank_dtype == "mxfp4":
            for bank, f in zip(self._feats, feats):
                if tuple(f.shape[1:]) != (int(bank.data.shape[1]), self.dim):
                    raise ValueError(f"bank rows {tuple(f.shape[1:])} against {(int(bank.data.shape[1]), self.dim)}")
                if self._exact is not None and f.dtype != torch.bfloat16:
                    raise ValueError("an index with an exact store takes bf16 rows")
            rows = feats
            feats, scales = zip(*[mx_quantize_rows(f, MX_E2M1) for f in feats])
            if self._exact is not None:                                  # after the quantiser: it refuses non-finite rows
                for bank, f in zip(self._exact, rows):
                    bank.append(f)
            for bank, s in zip(self._scales, scales):
                bank.append(s)
        for bank, f in zip(self._feats, feats):
            bank.append(f)
        for bank, w in zip(self._weights, weights):
            if bank is not None:
                bank.append(w)
        self._append_groups(len(ids), groups)
        if self._alive is not None:
            self._alive.append(torch.ones((len(ids),), dtype=torch.bool, device=self.device))
        if self._positions is not None:
            for j, cid in enumerate(ids, len(self.ids)):
                self._positions.setdefault(cid, []).append(j)
        self.ids += ids

    # ------------------------------------------------------------------ persistence
    def save(self, path):
        """Formats 1 (features), 2 (fp8 codes), 3 (fp8 codes and the exact store), 4 (mxfp4 codes) and 5 (mxfp4 codes and the exact
        store). The token layout of a fused 'tva' bank (the one that
        cannot be inferred) travels as the extra key "token_layout", outside the fingerprint; files without the key are what they were.
        So do the selection's arrays: "alive" (bool [NB], only after a remove()), "groups" (int32 [NB]) and "group_labels" (only for an
        index with groups; labels a weights-only load admits: strings, numbers, tuples of them)."""
        if self.bank_dtype in _QUANTISED:
            mx = self.bank_dtype == "mxfp4"
            blob = {"format": "valor_amd.RetrievalIndex/4" if mx else "valor_amd.RetrievalIndex/2", "fingerprint": self.fingerprint(), "ids": self.ids,
                    "codes": [f.cpu().clone() for f in self.feats], "scales": [s.cpu().clone() for s in self.scales],
                    "weights": [w.cpu().clone() for w in self.weights]}
            if self.exact is not None:                                   # format 3 = format 2 + the exact store, format 5 = format 4 + it
                blob["format"] = "valor_amd.RetrievalIndex/5" if mx else "valor_amd.RetrievalIndex/3"
                blob["exact_feats"] = [e.cpu().clone() for e in self.exact_feats]
        else:
            blob = {"format": "valor_amd.RetrievalIndex/1", "fingerprint": self.fingerprint(), "ids": self.ids,
                    "feats": [f.cpu().clone() for f in self.feats], "weights": [None if w is None else w.cpu().clone() for w in self.weights]}
        if self._layout_saved:
            blob["token_layout"] = [[[m, n] for m, n in part] for part in self.token_layout]
        if self._removed:
            blob["alive"] = self.alive.cpu().clone()
        if self._groups is not None:
            blob["groups"], blob["group_labels"] = self.groups.cpu().clone(), list(self.group_labels)
        torch.save(blob, path)

    @classmethod
    def load(cls, path, device):
        blob = torch.load(path, map_location="cpu", weights_only=True)      # tensors, strings, numbers, lists and dicts only
        if not isinstance(blob, dict) or blob.get("format") not in tuple(f"valor_amd.RetrievalIndex/{n}" for n in (1, 2, 3, 4, 5)):
            raise ValueError(f"{path}: not a RetrievalIndex file")
        fp = blob["fingerprint"]
        if blob["format"].endswith(("/2", "/3", "/4", "/5")):
            third = blob["format"].endswith(("/3", "/5"))                 # with the exact store
            feature_dtype = {str(t): t for t in (torch.bfloat16, torch.float32)}.get(fp.get("dtype"))
            index = cls(fp["group"], fp["contra_type"], fp["late_fusion"], [c.to(device) for c in blob["codes"]],
                        [w.to(device) for w in blob["weights"]], blob["ids"], "mxfp4" if blob["format"].endswith(("/4", "/5")) else "fp8", scales=[s.to(device) for s in blob["scales"]], dtype=feature_dtype,
                        exact=fp.get("exact") if third else None, exact_feats=blob["exact_feats"] if third else None,
                        token_layout=blob.get("token_layout"))
        else:
            index = cls(fp["group"], fp["contra_type"], fp["late_fusion"], [f.to(device) for f in blob["feats"]],
                        [None if w is None else w.to(device) for w in blob["weights"]], blob["ids"], token_layout=blob.get("token_layout"))
        if index.fingerprint() != fp:
            raise ValueError(f"{path}: the stored tensors do not match the stored fingerprint {fp}")
        index._copy_selection(blob.get("alive"), blob.get("groups"), blob.get("group_labels"))
        return index

    def _copy_selection(self, alive, groups, labels):
        """take over another index's (or a file's) alive array, group ids and label table; None: the index has none"""
        NB = len(self.ids)
        if alive is not None:
            if tuple(alive.shape) != (NB,) or alive.dtype != torch.bool:
                raise ValueError(f"alive: a bool [{NB}] tensor")
            self._alive = _Bank(alive.to(self.device).clone())
            self._removed = NB - int(alive.sum())
        if groups is not None:
            labels = list(labels or ())
            if tuple(groups.shape) != (NB,) or groups.dtype != torch.int32 or (NB and int(groups.max()) >= len(labels)):
                raise ValueError(f"groups: an int32 [{NB}] tensor of ids into the {len(labels)} group_labels")
            self._groups = _Bank(groups.to(self.device).clone())
            self.group_labels, self._label_id = labels, {lab: g for g, lab in enumerate(labels)}

    # ------------------------------------------------------------------ queries
    @torch.no_grad()
    def encode_queries(self, model, batch_or_tokens):
        """The text side only: {'feat_t', 'mask', 'weight'} (mask / raw weight for a fine model). batch_or_tokens: a batch with
        'txt_tokens', the txt_tokens dict itself, or a token tensor [NQ, L] of the model's text encoder."""
        self._check_model(model)
        model.eval()
        q = batch_or_tokens
        if torch.is_tensor(q):
            q = {"bert_tokens": q, "clip_tokens": q}
        if "txt_tokens" not in q:
            q = {"txt_tokens": q}
        ev = model({"txt_tokens": q["txt_tokens"]}, task="ret%t", compute_loss=False)
        ft = ev["feat_t"]
        if self.contra_type == "coarse":
            return {"feat_t": ft}
        return {"feat_t": ft, "mask": (ev["txt_tokens"].to(ft.device) != 0).float(),
                "weight": None if self.unit_text_weights else E._fine_weights(model, "text", ft)}

    def _queries(self, model, q):
        """model None: q is already {'feat_t' [, 'mask', 'weight' (raw)]}"""
        if model is not None:
            q = self.encode_queries(model, q)
        ft = q["feat_t"]
        if not ft.is_cuda or not self.device.type == "cuda":
            raise lib.ValorHipError("RetrievalIndex.search needs the bank and the queries on the GPU (no CPU fallback)")
        dtype_ok = ft.dtype in (torch.bfloat16, torch.float32) if self.bank_dtype in _QUANTISED else ft.dtype == self.dtype
        if ft.shape[-1] != self.dim or not dtype_ok or ft.dim() != (3 if self.contra_type == "fine" else 2):
            raise ValueError(f"query features {tuple(ft.shape)} {ft.dtype} against a {self.contra_type} bank of D={self.dim}, {self.dtype}")
        ft = ft.contiguous()
        if self.contra_type == "coarse":
            return ft, None, None
        NQ, T = ft.shape[:2]
        f32 = dict(dtype=torch.float32, device=ft.device)
        mask = q.get("mask")
        mask = torch.ones((NQ, T), **f32) if mask is None else mask.to(ft.device).float().contiguous()
        raw = q.get("weight")
        if self.unit_text_weights and raw is not None:
            raise ValueError("late_fusion scores use unit text token weights: pass none")
        raw = torch.ones((NQ, T), **f32) if raw is None else raw.float().contiguous()
        wq = torch.empty((NQ, T), **f32)
        lib.call("valor_fine_weight_softmax", K._stream(), raw.data_ptr(), mask.data_ptr(), wq.data_ptr(), NQ, T)
        if self.bank_dtype == "fp8" and T > 64:
            raise ValueError("an fp8 bank scores queries of at most 64 tokens (valor_fine_fused_fwd_fp8)")
        if self.bank_dtype == "mxfp4" and T > 64:
            raise ValueError("an mxfp4 bank scores queries of at most 64 tokens (valor_fine_fused_fwd_mx)")
        return ft, mask, wq

    def _fused(self, ft, part):
        return E.fused_scores_ok(ft, self._feats[part].data)

    def default_chunk(self, NQ, T=1):
        """clips per chunk: the [NQ, chunk] fp32 scores and the chunk's feature slice stay under the byte limit of valor_fine_fused_fwd
        (evaluate._FUSED_BYTES); on the non-fused fine path the fp32 token similarities [NQ * T, chunk * Nv] stay under 1 GiB"""
        D = self._feats[0].data.shape[-1]
        per_clip = NQ * 4
        for part, b in enumerate(self._feats):
            tokens = b.data.shape[1] if self.contra_type == "fine" else 1
            per_clip = max(per_clip, tokens * D * b.data.element_size())
        chunk = (E._FUSED_BYTES - 1) // per_clip
        if self.contra_type == "fine" and self.bank_dtype is None:
            for part, b in enumerate(self._feats):
                if not (self.dtype == torch.bfloat16 and T <= 64 and b.data.shape[1] <= 64 and D % 64 == 0):
                    chunk = min(chunk, _GEMM_PATH_BYTES // (NQ * T * ((b.data.shape[1] + 7) // 8 * 8) * 4))
        chunk = int(max(1, min(chunk, max(1, len(self)))))
        # a multiple of 4 keeps the dense [NQ, chunk] score rows 16-byte aligned: valor_topk_rows reads them with 16-byte loads (only the
        # last, shorter chunk of a bank whose size is no multiple of 4 takes the 4-byte loads)
        return chunk // 4 * 4 if chunk >= 4 and chunk < len(self) else chunk

    def _score_part(self, part, ft, mask, wq, c0, nb, ones, out):
        """out [NQ, nb] (dense fp32) = the scores of clips [c0, c0 + nb) of one bank part; ones: the clips' all-ones token mask [nb, Nv]"""
        fb = self._feats[part].data[c0:c0 + nb]
        if self.bank_dtype == "fp8":                                     # ft = the queries' (codes, scales)
            _scores_fp8(ft[0], ft[1], fb, self._scales[part].data[c0:c0 + nb], mask, ones, wq, self._weights[part].data[c0:c0 + nb], out)
            return
        if self.bank_dtype == "mxfp4":                                   # ft = the queries' (MX e4m3 codes, scale bytes)
            _scores_mx(ft[0], ft[1], fb, self._scales[part].data[c0:c0 + nb], mask, ones, wq, self._weights[part].data[c0:c0 + nb], out)
            return
        if self.contra_type == "coarse":
            K.gemm(ft, fb, out=out, out_dtype=torch.float32)
            return
        wb = self._weights[part].data[c0:c0 + nb]
        # the kernels of evaluate.fine_score_matrix / compute_fine_matrix, with the bank's weights already softmaxed
        (E._scores_fused if self._fused(ft, part) else E._scores_gemm)(ft, fb, mask, ones, wq, wb, out=out)

    def _chunks(self, ft, mask, wq, chunk):
        """yield (c0, scores [NQ, nb]) over the bank; the score tensor is a view of one reused buffer"""
        NQ, NB = ft.shape[0], len(self)
        chunk = self.default_chunk(NQ, ft.shape[1] if ft.dim() == 3 else 1) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("chunk >= 1")
        chunk = min(chunk, max(NB, 1))
        bufs = [torch.empty((NQ * chunk,), dtype=torch.float32, device=ft.device) for _ in self._feats]
        # the clips' token mask is all ones: one tensor per part for the whole walk, a chunk reads its leading rows
        ones = [torch.ones((chunk, b.data.shape[1]), dtype=torch.float32, device=ft.device) if self.contra_type == "fine" else None
                for b in self._feats]
        if self.bank_dtype == "fp8":
            ft = quantize_rows(ft)                                       # the query rows, once per call
        if self.bank_dtype == "mxfp4":
            ft = mx_quantize_rows(ft, MX_E4M3)                           # the query rows, once per call, to MX e4m3
        for c0 in range(0, NB, chunk):
            nb = min(chunk, NB - c0)
            outs = [b[:NQ * nb].view(NQ, nb) for b in bufs]
            for part, out in enumerate(outs):
                self._score_part(part, ft, mask, wq, c0, nb, None if ones[part] is None else ones[part][:nb], out)
            if len(outs) == 2:
                outs[0].add_(outs[1])                                    # late fusion: the tv and ta scores added (test.py:571-579)
            yield c0, outs[0]

    # ------------------------------------------------------------------ pair scores
    def _pair_store(self):
        """the bf16 feature store per part that pair scores read, or ValueError with the reason (there is no fallback)"""
        if self.contra_type != "fine":
            raise ValueError("pair scores cover fine banks only (a coarse score is one GEMM row: use scores())")
        if self.bank_dtype in _QUANTISED:
            if self._exact is None:
                raise ValueError(f"this {self.bank_dtype} bank keeps no exact store (build it with exact='device' or exact='host'): its candidates cannot be "
                                 "re-scored exactly")
            return self._exact
        if self.dtype != torch.bfloat16:
            raise ValueError(f"pair scores cover bf16 banks only (valor_fine_score_pairs), this bank is {self.dtype}")
        return self._feats

    def _pair_queries(self, ft):
        store = self._pair_store()
        if ft.dtype != torch.bfloat16 or ft.shape[1] > 64 or ft.shape[2] % 64 or any(b.data.shape[1] > 64 for b in store):
            raise ValueError(f"pair scores take bf16 queries, D % 64 == 0 and at most 64 tokens on either side (valor_fine_score_pairs has no "
                             f"fallback), got {tuple(ft.shape)} {ft.dtype}")
        return store

    def _check_candidates(self, cand, NQ):
        if not torch.is_tensor(cand) or cand.dtype != torch.int64 or cand.dim() != 2 or cand.shape[0] != NQ or cand.device != self.device:
            raise ValueError(f"candidates: an int64 [{NQ}, C] tensor of bank indices on {self.device} (-1 = no candidate)")
        return cand.contiguous()

    def _pair_scores(self, ft, mask, wq, cand):
        """fp32 [NQ, C]: the exact scores of the bank indices cand (int64 [NQ, C] on the device; outside [0, NB): -inf), the parts of a
        late-fusion bank added. A host store costs one synchronisation: the indices are read back, their rows gathered into a pinned
        staging buffer and copied once; the kernel then reads the staging buffer with cand = arange."""
        out = None
        for store, ws, pairs in self._pair_operands(ft, cand):
            sc = score_pairs(ft, mask, wq, store, ws, pairs)
            out = sc if out is None else out.add_(sc)                    # late fusion: the tv and ta scores added, as the chunk path does
        return out

    def _pair_operands(self, ft, cand):
        """What a pair kernel reads, per bank part: (store bf16 [NS, Nv, D], its softmaxed weights [NS, Nv], candidates into that store).
        A bank or a "device" store is read in place; the rows of a "host" store are gathered into a pinned staging buffer and copied
        once (the one synchronisation: the indices are read back), and the candidates become positions in it. Pair scores and pair
        alignments share this."""
        store = self._pair_queries(ft)
        NQ, C = cand.shape
        NB = len(self)
        staged = self.exact == "host" and NQ * C
        if staged:
            ok = (cand >= 0) & (cand < NB)
            flat = torch.where(ok, cand, torch.zeros_like(cand)).view(-1)
            local = torch.where(ok, torch.arange(NQ * C, dtype=torch.int64, device=cand.device).view(NQ, C), torch.full_like(cand, -1))
            flat_host = flat.cpu()                                       # the one synchronisation of a host-store search
        for part, bank in enumerate(store):
            ws = self._weights[part].view()
            if staged:
                rows = (NQ * C,) + tuple(bank.data.shape[1:])
                if part not in self._stage or self._stage[part][0].shape[0] < NQ * C:          # one pair of buffers per part, reused
                    self._stage[part] = (_pinned_empty(rows, torch.bfloat16), torch.empty(rows, dtype=torch.bfloat16, device=cand.device))
                host, devbuf = self._stage[part][0][:NQ * C], self._stage[part][1][:NQ * C]
                torch.index_select(bank.view(), 0, flat_host, out=host)
                devbuf.copy_(host, non_blocking=True)
                yield devbuf, ws.index_select(0, flat), local
            else:
                yield bank.view(), ws, cand

    def _explain(self, ft, mask, wq, cand, sim):
        layouts = self.token_layout or [None] * len(self._feats)
        parts = [AlignmentPart(align_pairs(ft, mask, wq, store, ws, pairs, sim=sim), layout)
                 for (store, ws, pairs), layout in zip(self._pair_operands(ft, cand), layouts)]
        return Alignment(cand, parts)

    @torch.no_grad()
    def explain(self, model, batch_or_tokens, candidates, sim=False):
        """The token alignments of given bank indices: candidates int64 [NQ, C] on the device, -1 (or anything outside the bank) = an
        empty slot (score -inf, index bytes 255, zeros). Returns an Alignment: per bank part (one; video and audio under late_fusion,
        each with the part's stored weights) every query token's best clip token, every clip token's best query token, the part's
        score split over the tokens of either side and, with sim=True, the masked token similarities [NQ, C, T, Nv]. Coverage and
        refusals as rescore(): a bf16 fine bank is read directly, an fp8 bank through its exact store ("host": one synchronisation);
        coarse banks, fp32 banks and fp8 banks without a store raise ValueError. Queries as in search()."""
        self._pair_store()
        ft, mask, wq = self._queries(model, batch_or_tokens)
        return self._explain(ft, mask, wq, self._check_candidates(candidates, ft.shape[0]), bool(sim))

    @torch.no_grad()
    def rescore(self, model, batch_or_tokens, candidates):
        """The exact scores fp32 [NQ, C] of given bank indices: candidates int64 [NQ, C] on the device, -1 (or anything outside the bank)
        = no candidate, scored -inf. A bf16 fine bank is read directly, an fp8 bank through its exact store (a "host" store: one
        synchronisation per call); under late_fusion the two parts' pair scores are added. Coarse banks, fp32 banks and fp8 banks
        without a store raise ValueError. Queries as in search()."""
        self._pair_store()
        ft, mask, wq = self._queries(model, batch_or_tokens)
        return self._pair_scores(ft, mask, wq, self._check_candidates(candidates, ft.shape[0]))

    def _select_within(self, ft, mask, wq, cand, k, keep=None, group=None):
        """the k best of every row of candidates under the search's total order: (scores [NQ, k], bank indices [NQ, k]). keep (bool
        [NB] or [NQ, NB]): a candidate it rules out counts as -1; group (int32 [NB]): one result per group. Both are gathered per
        candidate position and go to valor_topk_rows_select; without them the selection is valor_topk_rows."""
        if cand.shape[1] == 0:                                           # an empty list: nothing to select from
            NQ = cand.shape[0]
            return (torch.full((NQ, k), float("-inf"), dtype=torch.float32, device=cand.device), torch.full((NQ, k), -1, dtype=torch.int64, device=cand.device))
        srt = within_prepare(cand, len(self))
        if keep is None and group is None:
            top_val, top_pos = topk_rows(self._pair_scores(ft, mask, wq, srt), k)
            return within_finish(top_val, top_pos, srt)
        at = lambda table: (table[None].expand(srt.shape[0], -1) if table.dim() == 1 else table).gather(1, srt.clamp(min=0))
        if keep is not None:
            srt = torch.where(at(keep), srt, torch.full_like(srt, -1))
        group_pos = None if group is None else torch.where(srt >= 0, at(group), torch.full_like(srt, -1, dtype=torch.int32)).contiguous()
        top_val, top_pos = topk_rows_select(self._pair_scores(ft, mask, wq, srt), k, keep=(srt >= 0).contiguous(), group=group_pos)
        return within_finish(top_val, top_pos, srt)

    def _selection(self, where, collapse, NQ):
        """(keep, group) of a search: keep = the alive array ANDed with `where` (bool [NB] or [NQ, NB] on the device), or None when both
        are absent; group = the group ids when collapse. (None, None): the plain selection."""
        NB = len(self)
        keep = self.alive if self._removed else None
        if where is not None:
            if (not torch.is_tensor(where) or where.dtype != torch.bool or where.device != self.device
                    or tuple(where.shape) not in ((NB,), (NQ, NB))):
                raise ValueError(f"where: a bool [{NB}] or [{NQ}, {NB}] tensor on {self.device}")
            keep = where.contiguous() if keep is None else where & keep
        return keep, (self.groups if collapse else None)

    def default_shortlist(self, k):
        """candidates the fp8 (mxfp4) walk of a two-stage search returns for re-scoring when the caller names no number"""
        return min(MAX_SHORTLIST, (SHORTLIST_FACTOR_MX if self.bank_dtype == "mxfp4" else SHORTLIST_FACTOR) * int(k))

    @torch.no_grad()
    def search(self, model, batch_or_tokens, k, chunk=None, *, within=None, shortlist=None, explain=False, sim=False, where=None,
               collapse=False):
        """The k best clips of every query: SearchResult (ids: list of lists, on demand; scores, indices: device [NQ, k]), best first,
        equal scores in index order. model None: batch_or_tokens = {'feat_t', 'mask', 'weight'} holds encoded queries (feat_t [NQ, T, D]
        or [NQ, D]; the text mask and RAW token weights of a fine model, None = ones).
        within (int64 [NQ, C] on the device; -1 and repeats allowed): the k best of each query's own candidate list instead of the
        bank, by exact pair scores (rescore()'s coverage), in the same order; the bank is not walked.
        shortlist (an fp8 bank with an exact store): the fp8 walk returns `shortlist` candidates (k <= shortlist <= 256), they are
        re-scored on the exact features and the exact top k is returned with the exact scores. None = default_shortlist(k) = min(256,
        4 k) (an mxfp4 bank: min(256, 8 k), and the walk is the mxfp4 walk throughout); 0 = fp8 scores only, which is all an index without a store does. With a "host" store the shortlist indices are read back,
        their rows gathered and copied: ONE host synchronisation per search; with a "device" store there is none.
        explain=True (every path; explain()'s coverage, checked before anything runs): the result carries `.alignment`, the Alignment
        of exactly the returned indices (empty slots: 255 / 0), with the token similarities when sim=True. Scores and indices are
        those of the search without it, bit for bit: the alignment's own score is not substituted.
        where (bool [NB] for all queries or [NQ, NB] per query, on the device): only clips it admits are returned, on every path (an
        entry of a within= list it rules out counts as -1). Removed clips are ruled out the same way, always.
        collapse=True (an index with groups): one result per group, the group's best admitted clip; clips of no group stand for
        themselves. The result's `.groups` / `.group_labels` name the groups. In a two-stage search the first stage applies the filter
        and does NOT collapse (its scores are approximate: it must not choose a group's representative), so the shortlist counts
        clips, the second stage collapses the exact scores, and a result may hold fewer than k groups when few groups fill the
        shortlist: a larger `shortlist` is the remedy.
        With nothing removed, no where and no collapse the selection is valor_topk_rows, as it was; otherwise it is
        valor_topk_rows_select (csrc/search_select.hip) with the shared arrays, chunk by chunk."""
        if not 1 <= int(k) <= 256:
            raise ValueError("1 <= k <= 256 (valor_topk_rows)")
        k = int(k)
        if collapse and self._groups is None:
            raise ValueError("collapse=True: the index has no groups (from_features / add_features / build take them)")
        if shortlist is None:
            shortlist = self.default_shortlist(k) if (self._exact is not None and within is None) else 0
        shortlist = int(shortlist)
        if shortlist:
            if within is not None:
                raise ValueError("within= scores its candidates exactly already: no shortlist")
            if self._exact is None:
                raise ValueError(f"shortlist: a two-stage search needs {'an mxfp4' if self.bank_dtype == 'mxfp4' else 'an fp8'} bank with an "
                                 f"exact store (exact='device' or 'host')")
            if not k <= shortlist <= MAX_SHORTLIST:
                raise ValueError(f"k <= shortlist <= {MAX_SHORTLIST} (valor_topk_rows), got k={k}, shortlist={shortlist}")
        if within is not None or explain:
            self._pair_store()
        ft, mask, wq = self._queries(model, batch_or_tokens)
        NQ = ft.shape[0]
        if explain:
            self._pair_queries(ft)
        keep, group = self._selection(where, bool(collapse), NQ)
        gathered = lambda idx: None if self._groups is None else torch.where(idx >= 0, self.groups[idx.clamp(min=0)], torch.full_like(idx, -1, dtype=torch.int32))
        attach = lambda val, idx: SearchResult(val, idx, self.ids, self._explain(ft, mask, wq, idx, bool(sim)) if explain else None,
                                               gathered(idx), self.group_labels)
        if within is not None:
            return attach(*self._select_within(ft, mask, wq, self._check_candidates(within, NQ), k, keep, group))
        if shortlist:
            self._pair_queries(ft)
            k_out, k = k, shortlist
        top_val = torch.full((NQ, k), float("-inf"), dtype=torch.float32, device=ft.device)
        top_idx = torch.full((NQ, k), -1, dtype=torch.int64, device=ft.device)
        ws = None
        for c0, score in self._chunks(ft, mask, wq, chunk):
            need = topk_workspace_bytes(NQ, score.shape[1], k)                   # the select entry's workspace is the same
            if ws is None or ws.numel() < need:
                ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=ft.device)
            if keep is None and (group is None or shortlist):
                topk_rows(score, k, col_base=c0, state=(top_val, top_idx), workspace=ws)
            else:                                                        # a first stage filters and leaves the collapsing to the second
                topk_rows_select(score, k, col_base=c0, state=(top_val, top_idx), workspace=ws, keep=keep, group=None if shortlist else group,
                                 check_state=False)                      # the tables span the bank
        if shortlist:                                                    # the second stage: exact scores of the fp8 walk's candidates
            top_val, top_idx = self._select_within(ft, mask, wq, top_idx, k_out, keep, group)
        return attach(top_val, top_idx)

    @torch.no_grad()
    def scores(self, model, batch_or_tokens, chunk=None):
        """The full [NQ, NB] score matrix under the chunk plan of search(): for checks and for small banks."""
        ft, mask, wq = self._queries(model, batch_or_tokens)
        out = torch.empty((ft.shape[0], len(self)), dtype=torch.float32, device=ft.device)
        for c0, score in self._chunks(ft, mask, wq, chunk):
            out[:, c0:c0 + score.shape[1]] = score
        return out
