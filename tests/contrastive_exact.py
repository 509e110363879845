"""Host side of the exact contrastive tests (tests/test_contrastive_exact_gpu.py, tests/test_contrastive_exact_inputs_cpu.py): inputs for
which the fine-grained contrastive reduction (model/pretrain.py:191-211) has ONE right answer, the integer reference, the conditions under
which that claim holds, a census of the planted tie / sign / mask structure, and guarded output buffers. Nothing here touches the GPU
library at import time.

Why tolerance zero is legitimate. Token features are drawn from {-1, 0, +1}: exact in bf16, in e4m3 and in fp32. Every dot product is an
integer of magnitude <= D <= 512 and every fp32 partial sum of it is exact in any order, so the MFMA tile of the fused kernel, valor_gemm
and the fp8 pipe must agree to the bit. Masks are 0 / 1, the fp8 row scales powers of two, the (already softmaxed, as far as the kernels
know) token weights multiples of 2^-6 and the upstream gradient multiples of 2^-4: every product and every partial sum of the score, of
d(sims) and of the weight gradients is a short dyadic number that fp32 holds exactly. `check_exactness_conditions` asserts all of it per
case, so a case that stops being exact fails as a CASE, not as a kernel.

What is planted (`make_case`), with the feature dimensions split into 8 `common` dims, 4 text-only, 4 clip-only and D - 16 content dims:
  * duplicate clip tokens v' = v + 1 (same lane quad), v + 4, v + 8 (other lane groups fg), v + 16, v + 32 (same lane, other 16-block) and
    duplicate text tokens t' = t + 1, t + 7 (other lanes of the DPP row), t + 16, t + 32, t + 48 (same lane, other 16-block); a text
    token elsewhere copies the duplicated clip token (and the other way round), so the tie IS the row maximum;
  * all-negative rows: `neg` texts carry -1 on the common dims and at most 3 content entries, `pos` clips +1 on the common dims: every
    similarity of the pair is in [-11, -5]. Text / clip 0 have a full mask (the maximum is negative: padding must not win), text / clip 1
    a masked slot 0 (before the best real slot), text / clip 2 a masked last slot (after it): there the masked slot's 0 is the maximum;
  * zero ties: tokens supported on the text-only (clip-only) dims have similarity exactly 0 with everything, tying with masked slots
    on either side;
  * masks on both sides: full, prefixes of length >= 1, interior holes, a masked slot 0."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

CANARY = -320.0               # float guard value: outside every result, exact in bf16
CANARY_U8 = 0xA5              # byte guard value: no arg-max byte (< 64) and not the prefill
PREFILL_U8 = 0x4D             # "never written" for arg-max bytes; floats are prefilled with NaN
COMMON, TEXT_ONLY, CLIP_ONLY, CONTENT0 = slice(0, 8), slice(8, 12), slice(12, 16), 16
DUP_B = ((0, 1), (2, 6), (3, 11), (4, 20), (5, 37))          # clip tokens: v' = v + 1, + 4, + 8, + 16, + 32
DUP_A = ((0, 1), (2, 9), (3, 19), (4, 36), (5, 53))          # text tokens: t' = t + 1, + 7, + 16, + 32, + 48
LINK_A = (6, 7, 8, 10, 11)                                    # text slot LINK_A[j] copies the clip token DUP_B[j][0]
LINK_B = (7, 8, 9, 10, 12)                                    # clip slot LINK_B[j] copies the text token DUP_A[j][0]
ZERO_A, ZERO_B = (12, 13, 44, 45), (13, 14)                   # zero-similarity tokens of regular texts / plain clips


def pad_blocks(n):
    """the dispatch rule of valor_fine_fused_fwd / _fp8: token slots padded to 16 * pad_blocks(n)"""
    return 1 if n <= 16 else (2 if n <= 32 else 4)


@dataclass(frozen=True)
class Shape:
    name: str
    NA: int
    NB: int
    T: int
    Nv: int
    D: int
    seed: int = 1

    @property
    def key(self):
        return (self.NA, self.NB, self.T, self.Nv, self.D, self.seed)


def _tile_counts(tpb, vpb):
    return 2 * (8 // tpb) + 1, 8 // vpb + 1         # NA = 2 RA + 1, NB = CB + 1: tile tails in both directions, grids of 3, 6, ... workgroups


def _fused(name, T, Nv, D, seed):
    NA, NB = _tile_counts(pad_blocks(T), pad_blocks(Nv))
    return Shape(name, NA, NB, T, Nv, D, seed)


# all nine (TPB, VPB) instantiations; 1 / 15 / 16 / 17 / 32 / 33 / 64 on both axes; D = 64 and 128 (one and two K steps of the bf16 kernel)
FUSED_SHAPES = (
    _fused("t16_v15", 16, 15, 64, 1),        # (1, 1)
    _fused("t15_v17", 15, 17, 128, 2),       # (1, 2)
    _fused("t1_v33", 1, 33, 64, 3),          # (1, 4)
    _fused("t17_v16", 17, 16, 128, 4),       # (2, 1)
    _fused("t32_v32", 32, 32, 64, 5),        # (2, 2)
    _fused("t32_v64", 32, 64, 128, 6),       # (2, 4)
    _fused("t33_v1", 33, 1, 128, 7),         # (4, 1)
    _fused("t64_v17", 64, 17, 64, 8),        # (4, 2)
    _fused("t64_v33", 64, 33, 128, 9),       # (4, 4)
    _fused("t33_v64_d512", 33, 64, 512, 10),  # (4, 4), eight K steps
    Shape("rect_3x70", 3, 70, 17, 16, 128, 11),   # evaluation shape, NA << NB
)
# the e4m3 twin needs D % 128 == 0: the same token shapes at D = 128 (one K step) and the D = 512 case
FP8_SHAPES = tuple(s if s.D % 128 == 0 else Shape(s.name + "_d128", s.NA, s.NB, s.T, s.Nv, 128, s.seed + 100) for s in FUSED_SHAPES)
# backward tiles: lane = clip, 64 clips per wave -> NB on both sides of 64; Nv even (packed 4-byte stores when ldS is even too) and odd;
# Nv <= 16 and > 16 (the two register-array sizes of fine_ds_chunk_kernel)
BWD_SHAPES = (
    Shape("b63_t15_v16", 63, 63, 15, 16, 64, 21),
    Shape("b64_t17_v15", 64, 64, 17, 15, 64, 22),
    Shape("b65_t16_v32", 65, 65, 16, 32, 64, 23),
    Shape("b70_t33_v17", 70, 70, 33, 17, 64, 24),
)
# through the autograd functions of valor_amd.ops: B = 9, and B = 67 in three backward chunks of 32 with a partial last one
OPS_SHAPES = (Shape("ops_b9_t17_v16", 9, 9, 17, 16, 64, 31), Shape("ops_b67_t15_v10", 67, 67, 15, 10, 64, 32))
ALL_SHAPES = tuple({s.key: s for s in FUSED_SHAPES + FP8_SHAPES + BWD_SHAPES + OPS_SHAPES}.values())


class ExactCase:
    """numpy arrays of one case: featA [NA, T, D], featB [NB, Nv, D] (int8 in {-1, 0, 1}), maskA / maskB (0 / 1), wA / wB (multiples of
    2^-6), dscore [NA, NB] (multiples of 2^-4), scaleA / scaleB (powers of two, the fp8 row scales), kindA / kindB (item kinds)"""

    def __init__(self, shape, **arrays):
        self.shape = shape
        self.__dict__.update(arrays)

    @property
    def dims(self):
        s = self.shape
        return s.NA, s.NB, s.T, s.Nv, s.D


def _content_token(rng, D, nnz):
    tok = np.zeros(D, dtype=np.int8)
    pos = CONTENT0 + rng.choice(D - CONTENT0, size=nnz, replace=False)
    tok[pos] = rng.choice(np.array([-1, 1], dtype=np.int8), size=nnz)
    return tok


def _only_token(rng, D, where):
    tok = np.zeros(D, dtype=np.int8)
    tok[where] = rng.choice(np.array([-1, 1], dtype=np.int8), size=4)
    return tok


def _mask(n, kind, i):
    m = np.ones(n, dtype=np.float64)
    if n == 1 or kind == "full":
        return m
    if kind == "first":
        m[0] = 0
    elif kind == "last":
        m[n - 1] = 0
    elif kind == "prefix":
        m[max(1, n - 1 - i % max(1, n // 2)):] = 0
    elif kind == "holes":
        m[1] = 0
        m[n // 2] = 0
    elif kind == "first_prefix":
        m[0] = 0
        m[max(2, n - 2):] = 0
    return m


_REGULAR_MASKS = ("full", "prefix", "holes", "first_prefix")


def make_case(NA, NB, T, Nv, D, seed=1, name=None):
    assert D >= 64 and D % 64 == 0 and 1 <= T <= 64 and 1 <= Nv <= 64 and NA >= 2 and NB >= 3
    rng = np.random.default_rng(seed * 7919 + 13)
    nnz = int(round((3.0 * (D - CONTENT0)) ** 0.5))          # about three overlapping entries per token pair: similarities in -5 .. 5, many ties
    nneg = min(3, NA - 1)
    featA = np.zeros((NA, T, D), dtype=np.int8)
    featB = np.zeros((NB, Nv, D), dtype=np.int8)
    kindA = ["neg" if a < nneg else "regular" for a in range(NA)]
    kindB = ["plain" if (b >= 3 and (b % 4 == 3 or (Nv == 1 and b % 2 == 1))) else "pos" for b in range(NB)]
    # ---- base tokens
    for a in range(NA):
        for t in range(T):
            if kindA[a] == "neg":
                featA[a, t] = _content_token(rng, D, int(rng.integers(0, 4)))
                featA[a, t, COMMON] = -1
            else:
                featA[a, t] = _content_token(rng, D, nnz)
        if kindA[a] == "regular":
            for t in ZERO_A:
                if t < T:
                    featA[a, t] = _only_token(rng, D, TEXT_ONLY)
            if T == 1 and a % 2 == 0:
                featA[a, 0] = _only_token(rng, D, TEXT_ONLY)
    for b in range(NB):
        for v in range(Nv):
            featB[b, v] = _content_token(rng, D, nnz)
            if kindB[b] == "pos":
                featB[b, v, COMMON] = 1
        if kindB[b] == "plain":
            for v in ZERO_B:
                if v < Nv:
                    featB[b, v] = _only_token(rng, D, CLIP_ONLY)
            if Nv == 1:
                featB[b, 0] = _only_token(rng, D, CLIP_ONLY)
    # ---- links (from the base tokens of the duplicated slots 0 .. 5, content dims only), then the duplicates
    baseA, baseB = featA.copy(), featB.copy()
    nreg = NA - nneg
    for a in range(nneg, NA):
        for j, t in enumerate(LINK_A):
            src = DUP_B[j][0]
            if t < T and src < Nv:
                featA[a, t, CONTENT0:] = baseB[a % NB, src, CONTENT0:]
    for b in range(NB):
        for j, v in enumerate(LINK_B):
            src = DUP_A[j][0]
            if v < Nv and src < T:
                featB[b, v, CONTENT0:] = baseA[nneg + b % nreg, src, CONTENT0:]
    for (s, d) in DUP_A:
        if d < T:
            featA[:, d] = featA[:, s]
    for (s, d) in DUP_B:
        if d < Nv:
            featB[:, d] = featB[:, s]
    # ---- masks
    maskA = np.stack([_mask(T, ("full", "first", "last")[a] if a < nneg else _REGULAR_MASKS[(a - nneg) % 4], a) for a in range(NA)])
    maskB = np.stack([_mask(Nv, ("full", "first", "last")[b] if b < 3 else _REGULAR_MASKS[(b - 3) % 4], b) for b in range(NB)])
    # ---- weights (softmaxed as far as the kernels know: plain inputs, need not sum to 1), upstream gradient, fp8 row scales
    wA = rng.integers(0, 65, size=(NA, T)).astype(np.float64) / 64.0
    wB = rng.integers(0, 65, size=(NB, Nv)).astype(np.float64) / 64.0
    dscore = rng.integers(-32, 33, size=(NA, NB)).astype(np.float64) / 16.0
    scaleA = 2.0 ** -rng.integers(0, 4, size=(NA, T)).astype(np.float64)
    scaleB = 2.0 ** -rng.integers(0, 4, size=(NB, Nv)).astype(np.float64)
    scaleA.flat[0], scaleB.flat[0] = 1.0, 0.125
    if scaleA.size > 1:
        scaleA.flat[-1] = 0.125
    shape = Shape(name or f"{NA}x{NB}_t{T}_v{Nv}_d{D}", NA, NB, T, Nv, D, seed)
    return ExactCase(shape, featA=featA, featB=featB, maskA=maskA, maskB=maskB, wA=wA, wB=wB, dscore=dscore, scaleA=scaleA, scaleB=scaleB,
                     kindA=tuple(kindA), kindB=tuple(kindB))


@lru_cache(maxsize=None)
def case_for(shape):
    return make_case(shape.NA, shape.NB, shape.T, shape.Nv, shape.D, shape.seed, shape.name)


def dots_of(case):
    """the integer token x token dot products [NA, NB, T, Nv] (float64 holds them exactly)"""
    NA, NB, T, Nv, D = case.dims
    S = case.featA.reshape(NA * T, D).astype(np.float64) @ case.featB.reshape(NB * Nv, D).astype(np.float64).T
    return np.ascontiguousarray(S.reshape(NA, T, NB, Nv).transpose(0, 2, 1, 3))


def _reduce(x, wA, wB):
    A2B, idxA = x.max(axis=3), x.argmax(axis=3)               # np.argmax: the FIRST maximal index
    B2A, idxB = x.max(axis=2), x.argmax(axis=2)
    score = (np.einsum("abt,at->ab", A2B, wA) + np.einsum("abv,bv->ab", B2A, wB)) / 2.0
    return A2B, B2A, idxA, idxB, score


@lru_cache(maxsize=None)
def _reference_cached(shape):
    return reference(case_for(shape))


def reference_for(shape):
    return _reference_cached(shape)


def reference(case):
    """integer / fp64 reference of the forward (x, A2B, B2A, first arg max, score; score8 of the fp8 form) and of the backward for the
    upstream gradient case.dscore: dS [NA * T, NB * Nv], dwA, dwB. No autograd: the gradient is routed through idxA / idxB explicitly."""
    NA, NB, T, Nv, D = case.dims
    dots = dots_of(case)
    mA, mB = case.maskA, case.maskB
    x = dots * mA[:, None, :, None] * mB[None, :, None, :]
    A2B, B2A, idxA, idxB, score = _reduce(x, case.wA, case.wB)
    x8 = dots * (case.scaleA * mA)[:, None, :, None] * (case.scaleB * mB)[None, :, None, :]
    A2B8, B2A8, _, _, score8 = _reduce(x8, case.wA, case.wB)
    hitA = np.arange(Nv)[None, None, None, :] == idxA[:, :, :, None]                 # [a, b, t, v]: v == idxA[a, b, t]
    hitB = np.arange(T)[None, None, :, None] == idxB[:, :, None, :]                  # [a, b, t, v]: t == idxB[a, b, v]
    d = hitA * (case.wA * mA)[:, None, :, None] * mB[None, :, None, :] + hitB * (case.wB * mB)[None, :, None, :] * mA[:, None, :, None]
    dS4 = (case.dscore / 2.0)[:, :, None, None] * d
    dS = np.ascontiguousarray(dS4.transpose(0, 2, 1, 3)).reshape(NA * T, NB * Nv)
    dwA = 0.5 * np.einsum("ab,abt->at", case.dscore, A2B)
    dwB = 0.5 * np.einsum("ab,abv->bv", case.dscore, B2A)
    return dict(dots=dots, x=x, A2B=A2B, B2A=B2A, idxA=idxA, idxB=idxB, score=score, x8=x8, A2B8=A2B8, B2A8=B2A8, score8=score8,
                d=d, dS4=dS4, dS=dS, dwA=dwA, dwB=dwB)


def _is_multiple(x, unit):
    q = np.asarray(x, dtype=np.float64) / unit
    return bool(np.all(q == np.round(q)))


def _is_pow2(x):
    m, _ = np.frexp(np.asarray(x, dtype=np.float64))
    return bool(np.all(m == 0.5))


def check_exactness_conditions(case, ref=None):
    """the conditions under which the case has exactly one right answer in fp32 (bf16 for a bf16 d(sims))"""
    ref = ref or reference(case)
    NA, NB, T, Nv, D = case.dims
    name = case.shape.name
    LIM = 2.0 ** 24
    assert set(np.unique(case.featA)) <= {-1, 0, 1} and set(np.unique(case.featB)) <= {-1, 0, 1}, f"{name}: features are ternary"
    assert set(np.unique(case.maskA)) <= {0.0, 1.0} and set(np.unique(case.maskB)) <= {0.0, 1.0}
    assert bool((case.maskA.sum(1) >= 1).all()) and bool((case.maskB.sum(1) >= 1).all()), f"{name}: every item keeps a live token"
    # |dot|, and every partial sum of it over any k range in any order, is bounded by sum_k |a||b| <= D
    absdot = np.abs(case.featA.reshape(NA * T, D).astype(np.float64)) @ np.abs(case.featB.reshape(NB * Nv, D).astype(np.float64)).T
    assert float(absdot.max()) <= D <= 512 < LIM, f"{name}: |dot| reaches {absdot.max()}"
    assert _is_multiple(ref["dots"], 1.0)
    assert _is_multiple(case.wA, 2.0 ** -6) and _is_multiple(case.wB, 2.0 ** -6) and case.wA.min() >= 0 and case.wB.min() >= 0
    assert _is_multiple(case.dscore, 2.0 ** -4)
    assert _is_pow2(case.scaleA) and _is_pow2(case.scaleB), f"{name}: fp8 row scales are powers of two"
    assert len(np.unique(case.scaleA)) > 1 or case.scaleA.size == 1
    assert len(np.unique(case.scaleB)) > 1
    # score: every term max * w and every partial sum of the T + Nv terms, in any order, is a multiple of `gran` bounded by sum |terms|
    for tag, a2b, b2a, gran in (("bf16", ref["A2B"], ref["B2A"], 2.0 ** -6),
                                ("fp8", ref["A2B8"], ref["B2A8"], 2.0 ** -6 * float(case.scaleA.min()) * float(case.scaleB.min()))):
        ta = np.abs(a2b) * case.wA[:, None, :]
        tb = np.abs(b2a) * case.wB[None, :, :]
        assert _is_multiple(ta, gran) and _is_multiple(tb, gran), f"{name} {tag}: a score term is finer than {gran}"
        total = ta.sum(-1) + tb.sum(-1)
        assert float(total.max()) < LIM * gran, f"{name} {tag}: score partial sums reach {total.max()} at granularity {gran}"
        assert float(np.abs(a2b).max()) < LIM * gran * 64 and float(np.abs(b2a).max()) < LIM * gran * 64      # x itself (granularity 64 gran)
    # d(sims) = g * d: d = wA mA mB + wB mB mA is a multiple of 2^-6 (<= 2), g = dscore / 2 of 2^-5: the product is exact in fp32, so a
    # bf16 d(sims) must be the round-to-nearest-even of the exact value
    g = np.abs(case.dscore / 2.0)
    assert _is_multiple(ref["d"], 2.0 ** -6) and float(ref["d"].max()) <= 2.0
    assert float(g.max()) * 2.0 < LIM * 2.0 ** -11, f"{name}: g * d needs more than 24 bits"
    assert bool(np.all(ref["dS"].astype(np.float32).astype(np.float64) == ref["dS"])), f"{name}: d(sims) is not exact in fp32"
    # dwA = 0.5 * sum_b dscore * A2B: terms are multiples of 2^-4
    dsc = np.abs(case.dscore)[:, :, None]
    assert float((dsc * np.abs(ref["A2B"])).sum(axis=1).max()) < LIM * 2.0 ** -4, f"{name}: dwA partial sums are not exact"
    assert float((dsc * np.abs(ref["B2A"])).sum(axis=0).max()) < LIM * 2.0 ** -4, f"{name}: dwB partial sums are not exact"
    # the arg-max bytes fit, and the case is not vacuous: most scores are nonzero and no two texts / clips have the same score row / column
    assert int(ref["idxA"].max()) < 64 and int(ref["idxB"].max()) < 64
    assert float((ref["score"] != 0).mean()) > 0.5, f"{name}: the score matrix is mostly zero"
    assert float((ref["score8"] != 0).mean()) > 0.5
    return dict(absdot=float(absdot.max()), score_abs=float(np.abs(ref["score"]).max()))


def _lane_v(n):
    return (np.arange(n) % 16) // 4          # A2B: the lane group fg that holds clip token v (4 consecutive v per lane, per 16-block)


def _lane_t(n):
    return np.arange(n) % 16                 # B2A: the lane fr of the DPP row that holds text token t


def _axis_census(x, slot_mask, row_live, lane):
    """x [..., m, n]: rows reduced over the last axis. slot_mask broadcastable to x (1 = real slot), row_live broadcastable to x[..., 0]."""
    n = x.shape[-1]
    slot_mask = np.broadcast_to(slot_mask, x.shape) > 0
    row_live = np.broadcast_to(row_live, x.shape[:-1]) > 0
    mx = x.max(-1)
    i0 = x.argmax(-1)
    at_max = x == mx[..., None]
    first_real = np.take_along_axis(slot_mask, i0[..., None], -1)[..., 0]
    others = at_max & slot_mask & (np.arange(n) != i0[..., None])                    # other REAL slots that attain the maximum
    lane0 = lane[i0][..., None]
    blk = np.arange(n) // 16
    blk0 = (i0 // 16)[..., None]
    real_tie = row_live & first_real
    has_masked = (~slot_mask).any(-1)
    real_zero = (at_max & slot_mask).any(-1) & (mx == 0)
    return dict(
        same_lane_tie=int((real_tie & (others & (lane == lane0)).any(-1)).sum()),
        cross_lane_tie=int((real_tie & (others & (lane != lane0)).any(-1)).sum()),
        cross_block_tie=int((real_tie & (others & (blk != blk0)).any(-1)).sum()),
        negative_max=int((row_live & (mx < 0)).sum()),
        masked_is_max=int((row_live & ~first_real).sum()),
        negative_under_masked_max=int((row_live & ~first_real & ((x < 0) | ~slot_mask).all(-1)).sum()),
        zero_vs_masked=int((row_live & real_zero & has_masked).sum()),
        zero_masked_first=int((row_live & real_zero & has_masked & ~first_real).sum()),
        zero_real_first=int((row_live & real_zero & has_masked & first_real).sum()),
    )


def census(case, ref=None):
    """how often each planted class occurs in the reference, per axis ("A2B": rows (a, b, t) reduced over v; "B2A": rows (a, b, v) reduced
    over t) and pooled ("all"). A row counts only if its own token is live; a tie only between REAL (unmasked) slots, the first of which is
    the arg max. same_lane_tie: the partner sits in the lane of the arg max (the in-lane scan decides); cross_lane_tie: in another lane
    (the shuffle / DPP `min` over candidates decides); cross_block_tie: in another 16-slot block."""
    ref = ref or reference(case)
    NA, NB, T, Nv, D = case.dims
    x = ref["x"]
    A = _axis_census(x, case.maskB[None, :, None, :], case.maskA[:, None, :], _lane_v(Nv))
    B = _axis_census(np.ascontiguousarray(x.transpose(0, 1, 3, 2)), case.maskA[:, None, None, :], case.maskB[None, :, :], _lane_t(T))
    return {"A2B": A, "B2A": B, "all": {k: A[k] + B[k] for k in A}}


def eligible_classes(T, Nv):
    """the classes a (T, Nv) shape admits at all: an axis of one slot has no ties, a cross-block tie needs more than 16 slots, a
    same-lane tie two clip tokens (one lane holds 4 consecutive v) or two text blocks (one lane holds t, t + 16, ...); a masked slot
    needs an axis of at least two (every item keeps a live token)."""
    cls = {"negative_max"}
    if Nv >= 2 or T > 16:
        cls.add("same_lane_tie")
    if Nv >= 5 or T >= 2:
        cls.add("cross_lane_tie")
    if Nv > 16 or T > 16:
        cls.add("cross_block_tie")
    if Nv >= 2 or T >= 2:
        cls |= {"masked_is_max", "negative_under_masked_max", "zero_vs_masked", "zero_masked_first", "zero_real_first"}
    return cls


# ------------------------------------------------------------------------------------------------ device side helpers (torch only)
def fp8_codes(feat):
    """the e4m3fn bytes of integer features in {-1, 0, 1} (uint8, same shape)"""
    return torch.from_numpy(feat.astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8)


def guarded(shape, dtype, dev, ld=None, margin=64):
    """(buf, view). A buffer filled with the guard value (-320, or 0xA5 for bytes) and a view of `shape` inside it, `margin` elements (1-D
    layout) or 2 rows (2-D with leading dimension `ld`) from either end, prefilled with "never written": NaN, or 0x4D for bytes."""
    is_u8 = dtype == torch.uint8
    fill, pre = (CANARY_U8, PREFILL_U8) if is_u8 else (CANARY, float("nan"))
    if ld is None:
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * margin,), fill, dtype=dtype, device=dev)
        view = buf[margin:margin + n].view(*shape)
    else:
        rows, cols = shape
        assert ld >= cols
        buf = torch.full((rows + 4, ld), fill, dtype=dtype, device=dev)
        view = buf[2:2 + rows, :cols]
    view.fill_(pre)
    return buf, view


def guard_intact(buf, view):
    """True if every element of `buf` outside `view` still holds the guard value"""
    b = buf.detach().cpu()
    inside = torch.zeros(b.shape, dtype=torch.bool)
    off = view.storage_offset() - buf.storage_offset()
    if b.dim() == 1:
        inside[off:off + view.numel()] = True
    else:
        r0, c0 = divmod(off, buf.stride(0))
        inside[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = True
    fill = CANARY_U8 if b.dtype == torch.uint8 else CANARY
    return bool(((b.float() == fill) | inside).all())


def first_mismatch(got, want):
    """None, or a description of the first element of `got` that differs in VALUE from `want` (-0.0 equals +0.0, NaN equals nothing)"""
    g = got.detach().cpu().double()
    w = torch.as_tensor(np.asarray(want, dtype=np.float64)) if not torch.is_tensor(want) else want.detach().cpu().double()
    assert tuple(g.shape) == tuple(w.shape), (tuple(g.shape), tuple(w.shape))
    bad = ~(g == w)
    if not bool(bad.any()):
        return None
    ix = tuple(int(i) for i in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(g).sum())} NaN), first at {ix}: got {float(g[ix])!r} want {float(w[ix])!r}"
