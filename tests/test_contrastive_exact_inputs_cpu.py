"""The inputs of tests/test_contrastive_exact_gpu.py, proved on the CPU: every case has exactly one right answer in fp32 (the conditions of
contrastive_exact.check_exactness_conditions), holds every planted class of ties / negative rows / masked maxima often enough for a wrong
tie rule to show (a condition on the inputs, not a measurement), the integer reference agrees with fp64 torch math, the dot products do
not depend on the summation order, and the case table reaches every instantiation of the fused kernels."""
import numpy as np
import pytest
import torch

import contrastive_exact as CE

REQUIRED = ("same_lane_tie", "cross_lane_tie", "cross_block_tie", "negative_max", "zero_vs_masked", "masked_is_max")
SUBCLASSES = ("negative_under_masked_max", "zero_masked_first", "zero_real_first")
IDS = [s.name for s in CE.ALL_SHAPES]


@pytest.mark.parametrize("shape", CE.ALL_SHAPES, ids=IDS)
def test_case_is_exact_and_holds_every_planted_class(shape):
    case, ref = CE.case_for(shape), CE.reference_for(shape)
    CE.check_exactness_conditions(case, ref)
    cen = CE.census(case, ref)
    ok = CE.eligible_classes(shape.T, shape.Nv)
    for cls in REQUIRED:
        if cls in ok:
            assert cen["all"][cls] >= 8, (shape.name, cls, cen["A2B"][cls], cen["B2A"][cls])
    for cls in SUBCLASSES:                      # refinements of the classes above: both orders of the masked / real slot occur
        if cls in ok:
            assert cen["all"][cls] >= 1, (shape.name, cls)
    # on an axis long enough for it, each tie class occurs on THAT axis (A2B: shuffles over lane groups; B2A: the DPP row)
    if shape.Nv >= 17:
        assert min(cen["A2B"][c] for c in ("same_lane_tie", "cross_lane_tie", "cross_block_tie")) >= 8, cen["A2B"]
    if shape.T >= 17:
        assert min(cen["B2A"][c] for c in ("same_lane_tie", "cross_lane_tie", "cross_block_tie")) >= 8, cen["B2A"]
    if shape.T >= 2 and shape.Nv >= 2:
        assert cen["A2B"]["negative_max"] >= 1 and cen["B2A"]["negative_max"] >= 1
        assert cen["A2B"]["masked_is_max"] >= 8 and cen["B2A"]["masked_is_max"] >= 8


@pytest.mark.parametrize("shape", CE.ALL_SHAPES, ids=IDS)
def test_integer_reference_equals_fp64_torch_math(shape):
    """pretrain.py:191-211 as the other tests of this project restate it (einsum, the masks multiply, max) in fp64: same values; the
    reference's arg max attains the maximum and nothing before it does"""
    case, ref = CE.case_for(shape), CE.reference_for(shape)
    fa, fb = torch.from_numpy(case.featA).double(), torch.from_numpy(case.featB).double()
    mA, mB = torch.from_numpy(case.maskA), torch.from_numpy(case.maskB)
    wA, wB = torch.from_numpy(case.wA), torch.from_numpy(case.wB)
    logits = torch.einsum("atd,bvd->abtv", fa, fb)
    logits = logits * mA[:, None, :, None] * mB[None, :, None, :]
    a2b, b2a = logits.max(dim=-1)[0], logits.max(dim=-2)[0]
    score = (torch.einsum("abt,at->ab", a2b, wA) + torch.einsum("abv,bv->ab", b2a, wB)) / 2.0
    assert torch.equal(a2b, torch.from_numpy(ref["A2B"])) and torch.equal(b2a, torch.from_numpy(ref["B2A"]))
    assert torch.equal(score, torch.from_numpy(ref["score"]))
    x = logits.numpy()
    for vals, idx, axis in ((ref["A2B"], ref["idxA"], 3), (ref["B2A"], ref["idxB"], 2)):
        at = np.take_along_axis(x, np.expand_dims(idx, axis), axis).squeeze(axis)
        assert np.array_equal(at, vals)
        n = x.shape[axis]
        shape_ix = [1, 1, 1, 1]
        shape_ix[axis] = n
        before = np.arange(n).reshape(shape_ix) < np.expand_dims(idx, axis)
        assert not bool((before & (x >= np.expand_dims(vals, axis))).any()), "an earlier slot attains the maximum"
    # the fp8 form: the dequantised rows code * scale through the same math
    l8 = torch.einsum("atd,bvd->abtv", fa * torch.from_numpy(case.scaleA)[:, :, None], fb * torch.from_numpy(case.scaleB)[:, :, None])
    l8 = l8 * mA[:, None, :, None] * mB[None, :, None, :]
    s8 = (torch.einsum("abt,at->ab", l8.max(dim=-1)[0], wA) + torch.einsum("abv,bv->ab", l8.max(dim=-2)[0], wB)) / 2.0
    assert torch.equal(s8, torch.from_numpy(ref["score8"]))
    codes = CE.fp8_codes(case.featA)
    assert set(codes.unique().tolist()) <= {0x00, 0x38, 0xB8}              # e4m3fn 0, +1, -1
    assert torch.equal(codes.view(torch.float8_e4m3fn).float(), torch.from_numpy(case.featA).float())


def test_backward_reference_by_brute_force():
    """dS / dwA / dwB of the vectorised reference against the formula written as loops, on the two smallest cases"""
    for shape in CE.FUSED_SHAPES:
        if shape.name not in ("t1_v33", "t33_v1"):
            continue
        case, ref = CE.case_for(shape), CE.reference_for(shape)
        NA, NB, T, Nv, D = case.dims
        dS = np.zeros((NA * T, NB * Nv))
        dwA, dwB = np.zeros((NA, T)), np.zeros((NB, Nv))
        for a in range(NA):
            for b in range(NB):
                g = case.dscore[a, b] / 2
                x = ref["x"][a, b]
                for t in range(T):
                    v = int(np.argmax(x[t]))
                    dS[a * T + t, b * Nv + v] += g * case.wA[a, t] * case.maskA[a, t] * case.maskB[b, v]
                    dwA[a, t] += g * x[t, v]
                for v in range(Nv):
                    t = int(np.argmax(x[:, v]))
                    dS[a * T + t, b * Nv + v] += g * case.wB[b, v] * case.maskB[b, v] * case.maskA[a, t]
                    dwB[b, v] += g * x[t, v]
        assert np.array_equal(dS, ref["dS"]) and np.array_equal(dwA, ref["dwA"]) and np.array_equal(dwB, ref["dwB"])


@pytest.mark.parametrize("shape", CE.ALL_SHAPES, ids=IDS)
def test_dot_products_do_not_depend_on_the_summation_order(shape):
    """the order-independence claim itself: fp32 accumulation forward, reversed and blocked by 64 (block sums first, then their sum)
    gives the integer reference bit for bit (the first 96 text and clip tokens of the case)"""
    case, ref = CE.case_for(shape), CE.reference_for(shape)
    NA, NB, T, Nv, D = case.dims
    A = case.featA.reshape(NA * T, D)[:96].astype(np.float32)
    B = case.featB.reshape(NB * Nv, D)[:96].astype(np.float32)
    want = (A.astype(np.float64) @ B.astype(np.float64).T).astype(np.float32)
    full = ref["dots"].transpose(0, 2, 1, 3).reshape(NA * T, NB * Nv)[:96, :96]
    assert np.array_equal(want.astype(np.float64), full)

    def accumulate(ks):
        acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
        for k in ks:
            acc = (acc + A[:, k, None] * B[None, :, k]).astype(np.float32)
        return acc

    fwd, rev = accumulate(range(D)), accumulate(range(D - 1, -1, -1))
    blocked = np.zeros_like(fwd)
    for k0 in range(0, D, 64):
        blocked = (blocked + accumulate(range(k0, k0 + 64))).astype(np.float32)
    for got in (fwd, rev, blocked):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_case_table_reaches_every_instantiation():
    blocks = lambda n: 1 if n <= 16 else (2 if n <= 32 else 4)             # the dispatch rule of valor_fine_fused_fwd(_fp8): <= 16 -> 1, <= 32 -> 2, else 4
    nine = {(t, v) for t in (1, 2, 4) for v in (1, 2, 4)}
    for table in (CE.FUSED_SHAPES, CE.FP8_SHAPES):
        assert {(blocks(s.T), blocks(s.Nv)) for s in table} == nine
        for n in (1, 15, 16, 17, 32, 33, 64):
            assert any(s.T == n for s in table) and any(s.Nv == n for s in table), n
    for n in range(1, 65):
        assert CE.pad_blocks(n) == blocks(n)
    assert {s.D for s in CE.FUSED_SHAPES} == {64, 128, 512} and all(s.D % 128 == 0 for s in CE.FP8_SHAPES)
    # tile tails in both directions (NA = 2 RA + 1, NB = CB + 1 with RA = 8 / TPB, CB = 8 / VPB) and one rectangular NA << NB case
    for s in CE.FUSED_SHAPES:
        if s.name.startswith("rect"):
            assert s.NA * 16 < s.NB
        else:
            assert s.NA == 2 * (8 // blocks(s.T)) + 1 and s.NB == 8 // blocks(s.Nv) + 1
    assert {s.NB for s in CE.BWD_SHAPES} == {63, 64, 65, 70}
    assert {s.Nv % 2 for s in CE.BWD_SHAPES} == {0, 1} and {s.Nv <= 16 for s in CE.BWD_SHAPES} == {True, False}
    assert max(max(s.NA, s.NB) for s in CE.ALL_SHAPES) <= 70
