"""The contrastive kernels (contrastive_fused.hip, contrastive.hip, the e4m3 twin of search_fp8.hip) held to exact answers on tie-heavy
inputs. tests/contrastive_exact.py builds cases for which the reduction of model/pretrain.py:191-211 has ONE right answer in fp32 --
ternary features, 0 / 1 masks, dyadic weights and upstream gradients, duplicate tokens in every lane relation, all-negative rows with and
without masked slots, zero ties against masked slots -- and tests/test_contrastive_exact_inputs_cpu.py proves that on the CPU. Here
every output is compared element for element at tolerance zero (values: -0.0 equals +0.0) inside guarded buffers: the first-arg-max
bytes, the directional maxima, the scores (full mode, scores-only mode, the unfused GEMM + reduce path on bf16 and fp32 features, the
rectangular score entry, the fp8 pipe), d(sims) from both backward entries (fp32, and bf16 as the round-to-nearest-even of the exact
value; packed and scalar stores), the token-weight gradients. The kernels with transcendentals (token-weight softmax, InfoNCE) are held
to fp64 within 4 x the error of the same formulas in plain fp32 torch plus 2^-22 of the quantity's magnitude; each comparison prints a
PARITY line (profiles/contrastive_exact_parity.txt holds those of one run)."""
import numpy as np
import pytest
import torch

import contrastive_exact as CE

pytestmark = pytest.mark.gpu

F32 = torch.float32
_DEV_CACHE = {}


def _t(x, dev, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev).contiguous()


def _inputs(shape, dev, dtype):
    """device tensors of a case (shared between the tests, never written)"""
    key = (shape.key, str(dtype))
    if key not in _DEV_CACHE:
        c = CE.case_for(shape)
        _DEV_CACHE[key] = dict(fa=_t(c.featA, dev, dtype), fb=_t(c.featB, dev, dtype), maskA=_t(c.maskA, dev), maskB=_t(c.maskB, dev),
                               wA=_t(c.wA, dev), wB=_t(c.wB, dev), dscore=_t(c.dscore, dev))
    return _DEV_CACHE[key]


def _exact(got, want, what):
    msg = CE.first_mismatch(got, want)
    assert msg is None, f"{what}: {msg}"


def _five(NA, NB, T, Nv, dev):
    """guarded score, A2B, B2A, idxA, idxB: [(buf, view), ...]"""
    return [CE.guarded((NA, NB), F32, dev), CE.guarded((NA, NB, T), F32, dev), CE.guarded((NA, NB, Nv), F32, dev),
            CE.guarded((NA, NB, T), torch.uint8, dev), CE.guarded((NA, NB, Nv), torch.uint8, dev)]


def _check_five(outs, ref, B_a, B_b, what):
    names = ("score", "A2B", "B2A", "idxA", "idxB")
    for (buf, view), n in zip(outs, names):
        _exact(view, ref[n][:B_a, :B_b], f"{what} {n}")
        assert CE.guard_intact(buf, view), f"{what}: {n} written outside its range"


def _check_negative_and_masked_rows(case, ref, a2b, b2a, idxa, idxb):
    """restated on the kernel's output: where every real similarity of a row is negative and nothing is masked the maximum is that negative
    integer and the index a real slot; padding never wins (an index is always below the token count)"""
    NA, NB, T, Nv, D = case.dims
    a2b, b2a, idxa, idxb = a2b.cpu().numpy(), b2a.cpu().numpy(), idxa.cpu().numpy().astype(np.int64), idxb.cpu().numpy().astype(np.int64)
    assert idxa.max() < Nv and idxb.max() < T, "a padded slot is the arg max"
    negA, negB = ref["A2B"] < 0, ref["B2A"] < 0
    assert bool((a2b[negA] < 0).all()) and bool((a2b[negA] == np.round(a2b[negA])).all())
    assert bool((b2a[negB] < 0).all()) and bool((b2a[negB] == np.round(b2a[negB])).all())
    mB_at = np.take_along_axis(np.broadcast_to(case.maskB[None, :, None, :], ref["x"].shape), idxa[..., None], 3)[..., 0]
    mA_at = np.take_along_axis(np.broadcast_to(case.maskA[:, None, :, None], ref["x"].shape), idxb[:, :, None, :], 2)[:, :, 0, :]
    assert bool((mB_at[negA] == 1).all()) and bool((mA_at[negB] == 1).all()), "a negative maximum sits on a masked slot"


# ------------------------------------------------------------------------------------------------ forward, tolerance zero
@pytest.mark.parametrize("shape", CE.FUSED_SHAPES, ids=[s.name for s in CE.FUSED_SHAPES])
def test_fused_forward_is_exact(dev, shape):
    """valor_fine_fused_fwd, full mode and scores-only mode, against the integer reference: all nine (TPB, VPB) instantiations"""
    from valor_amd import lib
    from valor_amd.kernels import _ptr as p, _stream as st
    NA, NB, T, Nv, D = CE.case_for(shape).dims
    case, ref = CE.case_for(shape), CE.reference_for(shape)
    x = _inputs(shape, dev, torch.bfloat16)
    outs = _five(NA, NB, T, Nv, dev)
    (_, s1), (_, a1), (_, b1), (_, ia1), (_, ib1) = outs
    lib.call("valor_fine_fused_fwd", st(), p(x["fa"]), p(x["fb"]), p(x["maskA"]), p(x["maskB"]), p(x["wA"]), p(x["wB"]), p(s1), p(a1), p(b1),
             p(ia1), p(ib1), NA, NB, T, Nv, D)
    _check_five(outs, ref, NA, NB, "fused")
    _check_negative_and_masked_rows(case, ref, a1, b1, ia1, ib1)
    sbuf, s3 = CE.guarded((NA, NB), F32, dev)
    lib.call("valor_fine_fused_fwd", st(), p(x["fa"]), p(x["fb"]), p(x["maskA"]), p(x["maskB"]), p(x["wA"]), p(x["wB"]), p(s3), 0, 0, 0, 0,
             NA, NB, T, Nv, D)
    _exact(s3, ref["score"], "fused scores-only")
    assert torch.equal(s1, s3) and CE.guard_intact(sbuf, s3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", CE.FUSED_SHAPES, ids=[s.name for s in CE.FUSED_SHAPES])
def test_unfused_forward_is_exact(dev, shape, dtype):
    """valor_gemm (fp32 out) + valor_fine_reduce_fwd (square: the first min(NA, NB) texts and clips of the case) and valor_fine_scores
    (rectangular, the whole case) against the integer reference -- not against the fused sibling"""
    from valor_amd import kernels as K, lib
    from valor_amd.kernels import _ptr as p, _stream as st
    case, ref = CE.case_for(shape), CE.reference_for(shape)
    NA, NB, T, Nv, D = case.dims
    x = _inputs(shape, dev, dtype)
    ldS = (NB * Nv + 7) // 8 * 8 + 8
    Sbuf, S = CE.guarded((NA * T, NB * Nv), F32, dev, ld=ldS)
    K.gemm(x["fa"].view(NA * T, D), x["fb"].view(NB * Nv, D), out=S, out_dtype=F32)
    _exact(S, ref["dots"].transpose(0, 2, 1, 3).reshape(NA * T, NB * Nv), "S")
    assert CE.guard_intact(Sbuf, S)
    sbuf, s = CE.guarded((NA, NB), F32, dev)
    lib.call("valor_fine_scores", st(), p(S), ldS, p(x["maskA"]), p(x["maskB"]), p(x["wA"]), p(x["wB"]), p(s), NA, NB, T, Nv)
    _exact(s, ref["score"], "valor_fine_scores")
    assert CE.guard_intact(sbuf, s)
    B = min(NA, NB)
    outs = _five(B, B, T, Nv, dev)
    (_, s2), (_, a2), (_, b2), (_, ia2), (_, ib2) = outs
    lib.call("valor_fine_reduce_fwd", st(), p(S), ldS, p(x["maskA"]), p(x["maskB"]), p(x["wA"]), p(x["wB"]), p(s2), p(a2), p(b2), p(ia2), p(ib2),
             B, T, Nv)
    _check_five(outs, ref, B, B, "reduce_fwd")


@pytest.mark.parametrize("shape", CE.FP8_SHAPES, ids=[s.name for s in CE.FP8_SHAPES])
def test_fp8_scores_are_exact(dev, shape):
    """valor_fine_fused_fwd_fp8 on the e4m3fn codes of the same integers with power-of-two row scales (2^-3 .. 2^0, not all equal): the
    score is scaleA scaleB x the integer dot through the same reduction, exactly; all nine instantiations"""
    from valor_amd import lib
    from valor_amd.kernels import _ptr as p, _stream as st
    case, ref = CE.case_for(shape), CE.reference_for(shape)
    NA, NB, T, Nv, D = case.dims
    x = _inputs(shape, dev, torch.bfloat16)
    ca, cb = CE.fp8_codes(case.featA).to(dev).contiguous(), CE.fp8_codes(case.featB).to(dev).contiguous()
    sA, sB = _t(case.scaleA, dev), _t(case.scaleB, dev)
    sbuf, s = CE.guarded((NA, NB), F32, dev)
    lib.call("valor_fine_fused_fwd_fp8", st(), p(ca), p(sA), p(cb), p(sB), p(x["maskA"]), p(x["maskB"]), p(x["wA"]), p(x["wB"]), p(s),
             NA, NB, T, Nv, D)
    _exact(s, ref["score8"], "fp8 score")
    assert CE.guard_intact(sbuf, s)


# ------------------------------------------------------------------------------------------------ backward, tolerance zero
def _rne(want, dtype):
    w = torch.from_numpy(np.ascontiguousarray(want)).to(F32)          # exact: check_exactness_conditions
    return w.to(dtype).double()


BWD_ALL = CE.BWD_SHAPES + tuple(s for s in CE.FUSED_SHAPES if s.name.startswith("rect"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", BWD_ALL, ids=[s.name for s in BWD_ALL])
def test_backward_tiles_are_exact(dev, shape, dtype):
    """valor_fine_reduce_bwd (square cases) and valor_fine_ds_chunk (chunks a0 = 0, interior, last partial) from the reference's arg-max
    bytes: every d(sims) element equals dscore / 2 ([v = idxA] wA mA mB + [t = idxB] wB mB mA), in bf16 its round-to-nearest-even; an
    even and an odd leading dimension for even Nv (packed 4-byte stores / scalar stores); the ld padding untouched; dwA / dwB from both
    entries exact; the element of a masked slot that is the maximum is exactly 0."""
    from valor_amd import kernels as K, lib
    from valor_amd.kernels import _ptr as p, _stream as st
    case, ref = CE.case_for(shape), CE.reference_for(shape)
    NA, NB, T, Nv, D = case.dims
    x = _inputs(shape, dev, torch.bfloat16)
    idxA, idxB = _t(ref["idxA"], dev, torch.uint8), _t(ref["idxB"], dev, torch.uint8)
    A2B, B2A = _t(ref["A2B"], dev), _t(ref["B2A"], dev)
    want = _rne(ref["dS"], dtype)
    ch = 24 if NA > 3 else 1
    chunks = [(0, min(ch, NA)), (ch, min(ch, NA - ch)), ((NA - 1) // ch * ch, NA - (NA - 1) // ch * ch)]
    assert chunks[-1][0] + chunks[-1][1] == NA and (NA <= 3 or chunks[-1][1] < ch)
    # a masked slot that is the maximum (and every other masked position) carries exactly 0
    mAB = case.maskA[:, None, :, None] * case.maskB[None, :, None, :]
    dead = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mAB == 0, ref["x"].shape).transpose(0, 2, 1, 3)).reshape(NA * T, NB * Nv))
    assert bool(dead.any()) and float(want[dead].abs().max()) == 0.0
    for extra in ((2, 3) if Nv % 2 == 0 else (3,)):
        ldS = NB * Nv + extra
        what = f"{shape.name} {dtype} ldS {ldS}"
        if NA == NB:
            dbuf, dS = CE.guarded((NA * T, NB * Nv), dtype, dev, ld=ldS)
            (wab, dwA), (wbb, dwB) = CE.guarded((NA, T), F32, dev), CE.guarded((NB, Nv), F32, dev)
            lib.call("valor_fine_reduce_bwd", st(), K.dt_of(dS), p(x["dscore"]), p(x["maskA"]), p(x["maskB"]), p(x["wA"]), p(x["wB"]), p(A2B), p(B2A),
                     p(idxA), p(idxB), p(dS), ldS, p(dwA), p(dwB), NA, T, Nv)
            _exact(dS, want, what + " reduce_bwd dS")
            assert float(dS.float().cpu()[dead].abs().max()) == 0.0
            _exact(dwA, ref["dwA"], what + " reduce_bwd dwA")
            _exact(dwB, ref["dwB"], what + " reduce_bwd dwB")
            assert CE.guard_intact(dbuf, dS) and CE.guard_intact(wab, dwA) and CE.guard_intact(wbb, dwB), what
        for a0, na in chunks:
            dbuf, dS = CE.guarded((na * T, NB * Nv), dtype, dev, ld=ldS)
            lib.call("valor_fine_ds_chunk", st(), K.dt_of(dS), p(x["dscore"]), p(x["maskA"]), p(x["maskB"]), p(x["wA"]), p(x["wB"]), p(idxA), p(idxB),
                     p(dS), ldS, a0, na, NB, T, Nv)
            _exact(dS, want[a0 * T:(a0 + na) * T], what + f" ds_chunk a0 {a0} na {na}")
            assert CE.guard_intact(dbuf, dS), what + f" ds_chunk a0 {a0}: written outside the tile"
    if NA == NB:
        (wab, dwA), (wbb, dwB) = CE.guarded((NA, T), F32, dev), CE.guarded((NB, Nv), F32, dev)
        lib.call("valor_fine_weight_grad", st(), p(x["dscore"]), p(A2B), p(B2A), p(dwA), p(dwB), NA, T, Nv)
        _exact(dwA, ref["dwA"], "weight_grad dwA")
        _exact(dwB, ref["dwB"], "weight_grad dwB")
        assert CE.guard_intact(wab, dwA) and CE.guard_intact(wbb, dwB)


# ------------------------------------------------------------------------------------------------ fp64 parity (transcendentals)
FLOOR = 2.0 ** -22
TINY = 2.0 ** -126          # results under the normal range may be flushed


def _parity(name, got, want64, plain32, mag):
    """|got - fp64| <= (4 r32 + 2^-22) mag elementwise, r32 = the largest error of the same formulas in plain fp32 torch on the same inputs,
    measured in units of `mag` (the magnitude of the quantity, elementwise or one number). Prints the measured pair."""
    got, want64, plain32 = got.detach().cpu().double(), want64.double(), plain32.double()
    mag = torch.as_tensor(mag, dtype=torch.float64).expand_as(want64)
    assert got.shape == want64.shape and bool(torch.isfinite(got).all()), name

    def units(err):
        r = torch.where(mag > 0, err / mag.clamp_min(1e-300), torch.where(err > TINY, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        return float(r.max()) if r.numel() else 0.0

    e32, ek = (plain32 - want64).abs(), (got - want64).abs()
    r32, rk = units(e32), units(ek)
    print(f"PARITY {name}: kernel {rk:.3e} plain-fp32 {r32:.3e} (units of the quantity's magnitude)")
    bad = ek > (4.0 * r32 + FLOOR) * mag + TINY
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements off; kernel {rk:.3e} vs plain fp32 {r32:.3e} (allowed {4 * r32 + FLOOR:.3e})"


def _softmax_math(raw, mask, dw, dtype):
    raw, mask, dw = raw.to(dtype), mask.to(dtype), dw.to(dtype)
    w = torch.softmax(raw.masked_fill(mask == 0, float("-inf")), dim=-1)
    draw = w * (dw - (w * dw).sum(-1, keepdim=True))
    return w, draw


@pytest.mark.parametrize("rows", [1, 5, 64])
@pytest.mark.parametrize("n", [1, 2, 63, 64])
def test_token_weight_softmax_against_fp64(dev, rows, n):
    """valor_fine_weight_softmax / _bwd: rows that are not a multiple of the 4 waves of a workgroup, n = 1 / 2 / 63 / 64; masks with one
    live slot (w exactly 1), a masked slot 0, interior holes; raw values N(0, 1), with +-1e4 offsets, all equal. Masked positions are
    exactly 0 forward and backward."""
    from valor_amd import lib
    from valor_amd.kernels import _ptr as p, _stream as st
    g = torch.Generator().manual_seed(rows * 100 + n)
    for values in ("normal", "offsets", "equal"):
        raw = torch.randn((rows, n), generator=g)
        if values == "offsets":
            raw = raw + torch.tensor([1e4, -1e4, 0.0])[torch.randint(0, 3, (rows, n), generator=g)]
        elif values == "equal":
            raw = torch.full((rows, n), 3.25)
        mask = torch.ones((rows, n))
        for r in range(rows):
            kind = r % 4
            if kind == 0:                                   # a single live slot
                mask[r] = 0
                mask[r, (r * 7) % n] = 1
            elif kind == 1 and n > 1:                       # a leading masked slot
                mask[r, 0] = 0
            elif kind == 2 and n > 2:                       # interior holes
                mask[r, 1::3] = 0
        dw = torch.randn((rows, n), generator=g)
        wbuf, w = CE.guarded((rows, n), F32, dev)
        dbuf, draw = CE.guarded((rows, n), F32, dev)
        raw_d, mask_d, dw_d = raw.to(dev), mask.to(dev), dw.to(dev)
        lib.call("valor_fine_weight_softmax", st(), p(raw_d), p(mask_d), p(w), rows, n)
        lib.call("valor_fine_weight_softmax_bwd", st(), p(w), p(dw_d), p(draw), rows, n)
        assert CE.guard_intact(wbuf, w) and CE.guard_intact(dbuf, draw)
        w64, _ = _softmax_math(raw, mask, dw, torch.float64)
        w32, draw32 = _softmax_math(raw, mask, dw, torch.float32)
        wk = w.cpu()
        assert float(wk[mask == 0].abs().sum()) == 0.0 and float(draw.cpu()[mask == 0].abs().sum()) == 0.0, "masked positions are exactly 0"
        single = mask.sum(-1) == 1
        assert bool((wk[single].sum(-1) == 1.0).all()) and bool((wk[single].max(-1)[0] == 1.0).all()), "a single live slot has weight exactly 1"
        _parity(f"softmax w rows={rows} n={n} {values}", wk, w64, w32, w64.abs())
        # the backward of the KERNEL's w (its input), in fp64
        draw64 = wk.double() * (dw.double() - (wk.double() * dw.double()).sum(-1, keepdim=True))
        mag = wk.double().abs() * (dw.double().abs() + (wk.double() * dw.double()).abs().sum(-1, keepdim=True))
        d32 = wk * (dw - (wk * dw).sum(-1, keepdim=True))
        _parity(f"softmax draw rows={rows} n={n} {values}", draw.cpu(), draw64, d32, mag)


def _infonce_math(score, k, g, dtype):
    """the kernels' formulas: lse = mx + log sum exp(k s - mx) per row / column; loss; ds = g / (2B) (p_r + p_c - 2 [a = b]); dscore = k ds;
    dk = sum ds s"""
    s, k, g = score.to(dtype), torch.tensor(k, dtype=dtype), torch.tensor(g, dtype=dtype)
    B = s.shape[0]
    z = k * s
    mr, mc = z.max(1, keepdim=True)[0], z.max(0, keepdim=True)[0]
    lse_r = (mr + torch.log(torch.exp(z - mr).sum(1, keepdim=True)))[:, 0]
    lse_c = (mc + torch.log(torch.exp(z - mc).sum(0, keepdim=True)))[0]
    loss = (lse_r + lse_c - 2 * z.diag()).sum() / (2 * B)
    ds = torch.exp(z - lse_r[:, None]) + torch.exp(z - lse_c[None, :]) - 2 * torch.eye(B, dtype=dtype)
    ds = ds * (g / (2 * B))
    return lse_r, lse_c, loss, k * ds, (ds * s).sum(), ds


def _check_infonce(dev, score, k, tag):
    from valor_amd import lib
    from valor_amd.kernels import _ptr as p, _stream as st
    B = score.shape[0]
    k32 = float(torch.tensor(k, dtype=F32))
    s_d, k_d = score.to(dev).contiguous(), torch.tensor(k, dtype=F32, device=dev)
    (rb, lse_r), (cb, lse_c), (lb, loss) = CE.guarded((B,), F32, dev), CE.guarded((B,), F32, dev), CE.guarded((1,), F32, dev)
    lib.call("valor_infonce_fwd", st(), p(s_d), p(k_d), p(lse_r), p(lse_c), p(loss), B)
    assert CE.guard_intact(rb, lse_r) and CE.guard_intact(cb, lse_c) and CE.guard_intact(lb, loss)
    for g in (1.0, -0.37):
        g32 = float(torch.tensor(g, dtype=F32))
        r64 = _infonce_math(score, k32, g32, torch.float64)
        r32 = _infonce_math(score, k32, g32, torch.float32)
        name = f"infonce {tag} B={B} k={k} g={g}"
        if g == 1.0:
            _parity(name + " lse_r", lse_r, r64[0], r32[0], r64[0].abs())
            _parity(name + " lse_c", lse_c, r64[1], r32[1], r64[1].abs())
            z = k32 * score.double()
            mag_loss = (r64[0].abs() + r64[1].abs() + 2 * z.diag().abs()).sum() / (2 * B)
            _parity(name + " loss", loss[0], r64[2], r32[2], mag_loss)
        g_d = torch.tensor(g, dtype=F32, device=dev)                  # the upstream gradient is read from the device
        (db, dscore), (kb, dk), (pb, part) = CE.guarded((B, B), F32, dev), CE.guarded((1,), F32, dev), CE.guarded((256,), F32, dev)
        lib.call("valor_infonce_bwd", st(), p(s_d), p(k_d), p(lse_r), p(lse_c), p(g_d), p(dscore), p(dk), p(part), B)
        assert CE.guard_intact(db, dscore) and CE.guard_intact(kb, dk) and CE.guard_intact(pb, part)
        _parity(name + " dscore", dscore, r64[3], r32[3], abs(g32) * abs(k32) / (2 * B))
        _parity(name + " dk", dk[0], r64[4], r32[4], float((r64[5] * score.double()).abs().sum()))


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257])
def test_infonce_against_fp64(dev, B):
    """valor_infonce_fwd / _bwd at B = 1, 2, around the 64 lanes of the statistics wave, and 257 (257^2 elements exceed the 256 x 256
    threads of the capped backward grid: the strided loop and the sum over 256 block partials run); k = 1, 14.285, 100; scores N(0, 0.1)
    with a boosted diagonal; upstream gradient 1 and -0.37 read from the device: lse_r, lse_c, loss, every dscore element, dk."""
    g = torch.Generator().manual_seed(1000 + B)
    score = 0.1 * torch.randn((B, B), generator=g) + 0.3 * torch.eye(B)
    for k in (1.0, 14.285, 100.0):
        _check_infonce(dev, score, k, "normal")


def test_infonce_wide_range(dev):
    """k * score spans +-2000: only the max-subtraction keeps expf finite"""
    B = 65
    g = torch.Generator().manual_seed(77)
    score = (torch.rand((B, B), generator=g) * 2 - 1) * 20.0
    score[0, 0], score[B - 1, 3] = 20.0, -20.0
    _check_infonce(dev, score, 100.0, "wide")


# ------------------------------------------------------------------------------------------------ through valor_amd.ops
# The integer features scaled by 2^-2 (similarities are multiples of 2^-4: still exact, the arg max still unambiguous), real-valued raw
# token weights and k, masks on both sides. The fp64 reference routes every gradient through the FIRST arg max explicitly (np.argmax of
# the exact similarities) -- not through autograd's tie choice. Feature gradients of bf16 runs: componentwise
# |got - want| <= 3 * 2^-8 * (|dS_ref| . |feat|): one rounding of d(sims) and one of the output, 2^-9 each, margin 1.5 (a sum of two bf16
# GEMM results, late fusion / two coarse operands, rounds a third time: 3 * 2^-9, still inside). Everything computed in fp32 (all of an
# fp32 run; loss, raw-weight gradients and dk of a bf16 run): the measured rule of _parity, the same math in plain fp32 torch.
OPS_K = 14.285
OPS_SCALE = 0.25
OPS_CHUNK = 32
_OPS_CACHE = {}


def _ops_inputs(shape, kind):
    """CPU fp64 inputs of an ops case: fa [B, T, D]; a list of B-side operands (fb, maskB, raw weights or None); maskA; raw text weights"""
    c = CE.case_for(shape)
    g = torch.Generator().manual_seed(shape.seed)
    fa = torch.from_numpy(c.featA).double() * OPS_SCALE
    fb = torch.from_numpy(c.featB).double() * OPS_SCALE
    mA, mB = torch.from_numpy(c.maskA).double(), torch.from_numpy(c.maskB).double()
    wa_raw, wb_raw = torch.randn(c.maskA.shape, generator=g).double(), torch.randn(c.maskB.shape, generator=g).double()
    G = (torch.randint(-32, 33, (shape.NA, shape.NB), generator=g).double() / 16.0)
    if kind == "fine":
        return dict(fa=fa, mA=mA, wa_raw=wa_raw, bs=[(fb, mB, wb_raw)], k=OPS_K, G=None)
    if kind == "score":
        return dict(fa=fa, mA=mA, wa_raw=None, bs=[(fb, mB, None)], k=None, G=G)
    if kind == "late":
        fb2 = torch.roll(fb, 2, dims=0).flip(1).contiguous()              # the second modality: other clips, token order reversed
        return dict(fa=fa, mA=mA, wa_raw=None, bs=[(fb, torch.ones_like(mB), None), (fb2, torch.ones_like(mB), None)], k=OPS_K, G=None)
    raise KeyError(kind)


def _fine_math(inp, dtype, idx=None):
    """compute_fine_matrix_slice (+ InfoNCE when k is given, else the upstream gradient G) and its gradients in `dtype`, every arg max taken
    from `idx` (first maximal index of the exact similarities; computed here when None). Returns (results, magnitudes, idx)."""
    cv = lambda t: None if t is None else t.to(dtype)
    fa, mA = cv(inp["fa"]), cv(inp["mA"])
    B, T, D = fa.shape
    ones_a = torch.ones((B, T), dtype=dtype)
    wA = torch.softmax((cv(inp["wa_raw"]) if inp["wa_raw"] is not None else ones_a).masked_fill(mA == 0, float("-inf")), -1)
    parts, out_idx = [], []
    score, score_mag = torch.zeros((B, B), dtype=dtype), torch.zeros((B, B), dtype=dtype)
    for j, (fb, mB, wb_raw) in enumerate(inp["bs"]):
        fb, mB = cv(fb), cv(mB)
        Nv = fb.shape[1]
        wB = torch.softmax((cv(wb_raw) if wb_raw is not None else torch.ones((B, Nv), dtype=dtype)).masked_fill(mB == 0, float("-inf")), -1)
        x = torch.einsum("atd,bvd->abtv", fa, fb) * mA[:, None, :, None] * mB[None, :, None, :]
        if idx is None:
            xn = x.numpy()
            iA, iB = torch.from_numpy(xn.argmax(3)), torch.from_numpy(xn.argmax(2))
        else:
            iA, iB = idx[j]
        out_idx.append((iA, iB))
        A2B = torch.gather(x, 3, iA[..., None])[..., 0]
        B2A = torch.gather(x, 2, iB[:, :, None, :])[:, :, 0, :]
        score = score + (torch.einsum("abt,at->ab", A2B, wA) + torch.einsum("abv,bv->ab", B2A, wB)) / 2
        score_mag = score_mag + (torch.einsum("abt,at->ab", A2B.abs(), wA) + torch.einsum("abv,bv->ab", B2A.abs(), wB)) / 2
        parts.append((fb, mB, wB, A2B, B2A, iA, iB, wb_raw is not None))
    res, mag = {}, {}
    if inp["k"] is not None:
        lse_r, lse_c, loss, dscore, dk, ds = _infonce_math(score, float(torch.tensor(inp["k"], dtype=F32)), 1.0, dtype)
        res["loss"], res["dk"] = loss, dk
        z = float(torch.tensor(inp["k"], dtype=F32)) * score
        mag["loss"] = (lse_r.abs() + lse_c.abs() + 2 * z.diag().abs()).sum() / (2 * B)
        mag["dk"] = (ds * score).abs().sum()
    else:
        dscore = cv(inp["G"])
        res["score"], mag["score"] = score, score_mag
    dfa, mag_dfa = torch.zeros_like(fa), torch.zeros_like(fa)
    dwA, mag_dwA = torch.zeros_like(wA), torch.zeros_like(wA)
    for j, (fb, mB, wB, A2B, B2A, iA, iB, has_w) in enumerate(parts):
        Nv = fb.shape[1]
        hitA = torch.nn.functional.one_hot(iA, Nv).to(dtype)                                  # [a, b, t, v]
        hitB = torch.nn.functional.one_hot(iB, T).to(dtype).permute(0, 1, 3, 2)               # [a, b, v, t] -> [a, b, t, v]
        d = hitA * (wA * mA)[:, None, :, None] * mB[None, :, None, :] + hitB * (wB * mB)[None, :, None, :] * mA[:, None, :, None]
        dS4 = (dscore / 2)[:, :, None, None] * d
        dfa = dfa + torch.einsum("abtv,bvd->atd", dS4, fb)
        res[f"dfb{j}"] = torch.einsum("abtv,atd->bvd", dS4, fa)
        mag_dfa = mag_dfa + torch.einsum("abtv,bvd->atd", dS4.abs(), fb.abs())
        mag[f"dfb{j}"] = torch.einsum("abtv,atd->bvd", dS4.abs(), fa.abs())
        dwA = dwA + 0.5 * torch.einsum("ab,abt->at", dscore, A2B)
        mag_dwA = mag_dwA + 0.5 * torch.einsum("ab,abt->at", dscore.abs(), A2B.abs())
        if has_w:
            dwB = 0.5 * torch.einsum("ab,abv->bv", dscore, B2A)
            mB_ = 0.5 * torch.einsum("ab,abv->bv", dscore.abs(), B2A.abs())
            res[f"dwb_raw{j}"] = wB * (dwB - (wB * dwB).sum(-1, keepdim=True))
            mag[f"dwb_raw{j}"] = wB * (mB_ + (wB * mB_).sum(-1, keepdim=True))
    res["dfa"], mag["dfa"] = dfa, mag_dfa
    if inp["wa_raw"] is not None:
        res["dwa_raw"] = wA * (dwA - (wA * dwA).sum(-1, keepdim=True))
        mag["dwa_raw"] = wA * (mag_dwA + (wA * mag_dwA).sum(-1, keepdim=True))
    return res, mag, out_idx


def _ops_reference(shape, kind):
    key = (shape.key, kind)
    if key not in _OPS_CACHE:
        inp = _ops_inputs(shape, kind)
        r64, mag, idx = _fine_math(inp, torch.float64)
        r32, _, _ = _fine_math(inp, torch.float32, idx)
        _OPS_CACHE[key] = (inp, r64, r32, mag)
    return _OPS_CACHE[key]


def _check_ops(tag, got, r64, r32, mag, dtype):
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    for name in sorted(got):
        through_bf16 = dtype == torch.bfloat16 and name.startswith("df")
        if through_bf16:
            g, w, m = got[name].detach().cpu().double(), r64[name], mag[name]
            bad = (g - w).abs() > 3.0 * 2.0 ** -8 * m + TINY
            worst = float(((g - w).abs() / m.clamp_min(1e-300))[m > 0].max()) if bool((m > 0).any()) else 0.0
            print(f"PARITY {tag} {name}: kernel {worst:.3e} of |dS_ref| . |feat| (allowed {3 * 2.0 ** -8:.3e})")
            assert not bool(bad.any()), f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements off, worst {worst:.3e} of |dS_ref| . |feat|"
        else:
            _parity(f"{tag} {name}", got[name].float(), r64[name], r32[name], mag[name])


OPS_RUNS = [(e, d) for e in ("fine_fused", "fine_unfused", "fine_score", "late_fusion") for d in (torch.bfloat16, torch.float32)
            if not (e == "fine_fused" and d == torch.float32)]


@pytest.mark.parametrize("entry,dtype", OPS_RUNS, ids=[f"{e}-{'bf16' if d == torch.bfloat16 else 'fp32'}" for e, d in OPS_RUNS])
@pytest.mark.parametrize("shape", CE.OPS_SHAPES, ids=[s.name for s in CE.OPS_SHAPES])
def test_fine_ops_gradients_route_through_the_first_arg_max(dev, shape, entry, dtype):
    """ops.fine_contrastive (fused, three backward chunks at B = 67; and unfused), FineScoreFn, late_fusion_fine_contrastive: loss / score and
    every gradient element against the fp64 reference; gradients at masked text positions, and of their weights, are exactly 0"""
    from valor_amd import lib, ops
    kind = {"fine_fused": "fine", "fine_unfused": "fine", "fine_score": "score", "late_fusion": "late"}[entry]
    inp, r64, r32, mag = _ops_reference(shape, kind)
    leaf = lambda t, dt=F32: t.to(dt).to(dev).requires_grad_(True)
    fa = leaf(inp["fa"], dtype)
    fbs = [leaf(fb, dtype) for fb, _, _ in inp["bs"]]
    mA = inp["mA"].float().to(dev)
    mBs = [m.float().to(dev) for _, m, _ in inp["bs"]]
    so = lib.load()
    old_fused, old_chunk = so.valor_fine_set_fused(-1), ops._FINE_CHUNK
    got = {}
    try:
        so.valor_fine_set_fused(0 if entry == "fine_unfused" else 1)
        ops._FINE_CHUNK = OPS_CHUNK
        if kind == "fine":
            assert entry != "fine_fused" or (shape.NA + OPS_CHUNK - 1) // OPS_CHUNK == (3 if shape.NA == 67 else 1)
            wa, wb, k = leaf(inp["wa_raw"]), leaf(inp["bs"][0][2]), leaf(torch.tensor(OPS_K))
            loss = ops.fine_contrastive(fa, fbs[0], wa, wb, mA, mBs[0], k)
            loss.backward()
            got = dict(loss=loss.detach(), dk=k.grad, dfa=fa.grad, dfb0=fbs[0].grad, dwa_raw=wa.grad, dwb_raw0=wb.grad)
            assert float(wa.grad[mA == 0].abs().sum()) == 0.0 and float(wb.grad[mBs[0] == 0].abs().sum()) == 0.0
        elif kind == "score":
            score = ops.FineScoreFn.apply(fa, fbs[0], mA, mBs[0])
            (score * inp["G"].float().to(dev)).sum().backward()
            got = dict(score=score.detach(), dfa=fa.grad, dfb0=fbs[0].grad)
        else:
            k = leaf(torch.tensor(OPS_K))
            loss = ops.late_fusion_fine_contrastive(fa, fbs[0], fbs[1], mA, k)
            loss.backward()
            got = dict(loss=loss.detach(), dk=k.grad, dfa=fa.grad, dfb0=fbs[0].grad, dfb1=fbs[1].grad)
        torch.cuda.synchronize()
    finally:
        so.valor_fine_set_fused(old_fused)
        ops._FINE_CHUNK = old_chunk
    assert float(fa.grad.float()[mA == 0].abs().sum()) == 0.0, "a masked text position carries no gradient"
    assert float(fbs[0].grad.float()[mBs[0] == 0].abs().sum()) == 0.0, "a masked clip position carries no gradient"
    _check_ops(f"ops {entry} {shape.name} {dtype}", got, r64, r32, mag, dtype)


def _coarse_math(fa, fbs, k, dtype):
    fa, fbs = fa.to(dtype), [f.to(dtype) for f in fbs]
    B = fa.shape[0]
    fsum = sum(fbs[1:], fbs[0])
    score = fa @ fsum.t()
    lse_r, lse_c, loss, dscore, dk, ds = _infonce_math(score, float(torch.tensor(k, dtype=F32)), 1.0, dtype)
    res = dict(loss=loss, dk=dk, dfa=dscore @ fsum)
    z = float(torch.tensor(k, dtype=F32)) * score
    mag = dict(loss=(lse_r.abs() + lse_c.abs() + 2 * z.diag().abs()).sum() / (2 * B), dk=(ds * score).abs().sum(), dfa=dscore.abs() @ sum(f.abs() for f in fbs))      # the operands' products are rounded one by one, then added
    for j in range(len(fbs)):
        res[f"dfb{j}"], mag[f"dfb{j}"] = dscore.t() @ fa, dscore.abs().t() @ fa.abs()
    return res, mag


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", CE.OPS_SHAPES, ids=[s.name for s in CE.OPS_SHAPES])
def test_coarse_contrastive_against_fp64(dev, shape, nb, dtype):
    """ops.coarse_contrastive with one and two B-side operands on pooled integer features (token 0 of every item, scaled by 2^-2): the
    scores are exact, the loss and every gradient element against fp64"""
    from valor_amd import ops
    c = CE.case_for(shape)
    fa = torch.from_numpy(c.featA[:, 0]).double() * OPS_SCALE
    fbs = [torch.from_numpy(c.featB[:, j % shape.Nv]).double() * OPS_SCALE for j in (0, 2)][:nb]
    r64, mag = _coarse_math(fa, fbs, OPS_K, torch.float64)
    r32, _ = _coarse_math(fa, fbs, OPS_K, torch.float32)
    leaf = lambda t, dt=F32: t.to(dt).to(dev).requires_grad_(True)
    a, bs, k = leaf(fa, dtype), [leaf(f, dtype) for f in fbs], leaf(torch.tensor(OPS_K))
    loss = ops.coarse_contrastive(a, bs, k)
    loss.backward()
    got = dict(loss=loss.detach(), dk=k.grad, dfa=a.grad)
    for j, b in enumerate(bs):
        got[f"dfb{j}"] = b.grad
    _check_ops(f"ops coarse x{nb} {shape.name} {dtype}", got, r64, r32, mag, dtype)
