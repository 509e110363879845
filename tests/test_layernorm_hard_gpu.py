"""The fused LayerNorm kernels (csrc/layernorm.hip) and valor_colsum held to the element-wise fp64 bounds of tests/ln_hard_inputs.py:
 (A) hard rows (the seven row classes, the four dy classes), every family of test_layernorm_dropout_gpu.CASES plus fp32 at 100 columns, full
     form, all nine outputs; and the class rows themselves through the plain LayerNorm (variance below eps, constant rows), forward and backward;
 (B) the operand forms the model uses, one at a time, on hard rows;
 (C) the alignment rule ln_half_ok: one operand 8-byte but not 16-byte aligned sends variant 2 back to the one-wave-per-row kernels, bit for bit;
 (D) the smallest row counts at which a workgroup takes a second / third row group of the grid-stride loops, against fp64 on the device;
 (E) valor_colsum over row counts, widths (vector tail, scalar tail, second panel), leading dimensions, both dtypes, accumulate on and off;
     valor_colsum_finalize with an fp32 output;
 (F) argument refusals, return codes only.

Every test prints `PARITY ln hard <case> {output: largest observed / allowed}` before it asserts."""
import contextlib
import time

import pytest
import torch

import ln_hard_inputs as H
from test_layernorm_dropout_gpu import CASES, OFFSET, RPS, SEED, _case, _family, _row_scale, _setup, device_rng  # noqa: F401

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
ERR_ARG = -1            # VALOR_ERR_ARG of include/valor_hip.h


def _to(c, dev):
    for k, v in vars(c).items():
        if torch.is_tensor(v):
            setattr(c, k, v.to(dev))
    return c


def _eps(cols):
    return 1e-12 if cols == 768 else 1e-5


# ---------------------------------------------------------------------------------------------- (A) hard rows, every family
@pytest.mark.parametrize("rows", [37, 333])
@pytest.mark.parametrize("c", CASES + [_case("wave-fp32", 100, variant=0, dtype=F32)])
def test_hard_rows(dev, device_rng, c, rows):
    from valor_amd import kernels as K
    cols, p, dtype = c["cols"], c["p"], c["dtype"]
    rs = _row_scale(rows, dev) if c["scaled"] else None
    rps = RPS if c["scaled"] else 0
    kw = dict(p_drop=p, seed=SEED, offset=OFFSET, row_scale=rs, rows_per_scale=rps)
    full = _to(H.make_case(rows, cols, dtype, seed=100), dev)
    plain = _to(H.make_case(rows, cols, dtype, seed=200, bias=False, residual=False, dz_in=False), dev)
    eps = _eps(cols)
    with _setup(dev, device_rng, c):
        fwd = K.bdrln_fwd(full.x, full.bias, full.residual, full.gamma, full.beta, eps, **kw)
        bwd = K.bdrln_bwd(full.dy, full.dz_in, fwd[0], fwd[2], fwd[3], full.gamma, want_dbias=True, **kw)
        pf = K.bdrln_fwd(plain.x, None, None, plain.gamma, plain.beta, eps, write_z=False)
        pb = K.bdrln_bwd(plain.dy, None, plain.x, pf[2], pf[3], plain.gamma, want_dbias=True)
    keep = H.keep_mask(SEED, OFFSET + c["base"], rows, cols, p, dev)
    depth = H.bwd_depth(rows, cols, dtype, c["variant"])
    assert pf[0] is None and bwd[0].data_ptr() != bwd[1].data_ptr() and pb[0].data_ptr() == pb[1].data_ptr()
    items = H.forward_items(full, fwd, eps, keep, p, rs, rps) + H.backward_items(full, fwd[0], fwd[2], fwd[3], bwd, depth, keep, p, rs, rps)
    pitems = H.forward_items(plain, pf, eps) + H.backward_items(plain, plain.x, pf[2], pf[3], pb, H.bwd_depth(rows, cols, dtype, c["variant"], has_dz_in=False))
    errs = []
    for tag, it, cc in ((f"full {c} rows={rows}", items, full), (f"plain {c} rows={rows}", pitems, plain)):
        try:
            H.judge_all(tag, it, cc.cls)
        except AssertionError as e:
            errs.append(str(e))
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------- (B) operand forms
WIDTHS = [pytest.param((768, BF16, 0), id="bf16-768-wave"), pytest.param((768, BF16, 2), id="bf16-768-half"),
          pytest.param((128, BF16, 1), id="bf16-128"), pytest.param((768, F32, 1), id="fp32-768")]
ROWS_B, P_B = 37, 0.1


@contextlib.contextmanager
def _form(dev, w, **make):
    cols, dtype, variant = w
    c = _to(H.make_case(ROWS_B, cols, dtype, seed=300, **make), dev)
    c.eps, c.variant = _eps(cols), variant
    c.keep = H.keep_mask(SEED, OFFSET, ROWS_B, cols, P_B, dev)
    c.kw = dict(p_drop=P_B, seed=SEED, offset=OFFSET)
    c.depth = H.bwd_depth(ROWS_B, cols, dtype, variant, has_dy=c.dy is not None, has_dz_in=c.dz_in is not None)
    with _family(variant, 0):
        yield c


def _fwd(c, **kw):
    from valor_amd import kernels as K
    return K.bdrln_fwd(c.x, c.bias, c.residual, c.gamma, c.beta, c.eps, **{**c.kw, **kw})


def _bwd(c, z, mean, rstd, **kw):
    from valor_amd import kernels as K
    return K.bdrln_bwd(c.dy, c.dz_in, z, mean, rstd, c.gamma, **{"want_dbias": True, **c.kw, **kw})


@pytest.mark.parametrize("w", WIDTHS)
def test_form_plain_layernorm(dev, w):
    with _form(dev, w, bias=False, residual=False) as c:
        c.kw = {}
        out = _fwd(c, write_z=False)
    assert out[0] is None
    H.judge_all(f"plain {w}", H.forward_items(c, out, c.eps), c.cls)


@pytest.mark.parametrize("beta", [False, True], ids=["no-gamma-no-beta", "gamma-no-beta"])
@pytest.mark.parametrize("w", WIDTHS)
def test_form_without_affine(dev, w, beta):
    with _form(dev, w, gamma=beta, beta=False) as c:
        fwd = _fwd(c)
        bwd = _bwd(c, fwd[0], fwd[2], fwd[3])
    assert (c.gamma is None) == (not beta) and c.beta is None
    H.judge_all(f"affine gamma={beta} {w}", H.forward_items(c, fwd, c.eps, c.keep, P_B)
                + H.backward_items(c, fwd[0], fwd[2], fwd[3], bwd, c.depth, c.keep, P_B), c.cls)


@pytest.mark.parametrize("w", WIDTHS)
def test_form_bias_dropout_residual_only(dev, w):
    with _form(dev, w) as c:
        out = _fwd(c, want_y=False)
    assert out[1] is None and out[2] is None and out[3] is None
    H.judge_all(f"want_y=False {w}", H.forward_items(c, out, c.eps, c.keep, P_B), c.cls)


@pytest.mark.parametrize("w", WIDTHS)
def test_form_inplace_z(dev, w):
    with _form(dev, w) as c:
        ref = _fwd(c)
        xc = c.x.clone()
        c.x = xc
        out = _fwd(c, inplace_z=True)
    assert out[0].data_ptr() == xc.data_ptr()
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("absent", ["bias", "residual"])
@pytest.mark.parametrize("w", WIDTHS)
def test_form_without_bias_or_residual(dev, w, absent):
    with _form(dev, w, **{absent: False}) as c:
        fwd = _fwd(c)
        bwd = _bwd(c, fwd[0], fwd[2], fwd[3])
    assert getattr(c, absent) is None
    H.judge_all(f"no {absent} {w}", H.forward_items(c, fwd, c.eps, c.keep, P_B)
                + H.backward_items(c, fwd[0], fwd[2], fwd[3], bwd, c.depth, c.keep, P_B), c.cls)


@pytest.mark.parametrize("absent", ["dy", "dz_in"])
@pytest.mark.parametrize("w", WIDTHS)
def test_form_backward_without_dy_or_dz_in(dev, w, absent):
    with _form(dev, w, **{absent: False}) as c:
        fwd = _fwd(c)
        bwd = _bwd(c, *((None, None, None) if absent == "dy" else (fwd[0], fwd[2], fwd[3])))
    if absent == "dy":
        assert bwd[2] is None and bwd[3] is None and bwd[4] is not None
    H.judge_all(f"no {absent} {w}", H.backward_items(c, fwd[0], fwd[2], fwd[3], bwd, c.depth, c.keep, P_B), c.cls)


@pytest.mark.parametrize("separate", [False, True], ids=["p0-aliased", "separate_dx"])
@pytest.mark.parametrize("w", WIDTHS)
def test_form_no_dropout(dev, w, separate):
    with _form(dev, w) as c:
        c.kw = {}
        fwd = _fwd(c)
        bwd = _bwd(c, fwd[0], fwd[2], fwd[3], separate_dx=separate)
    if separate:
        assert bwd[0].data_ptr() != bwd[1].data_ptr() and torch.equal(bwd[0], bwd[1])
    else:
        assert bwd[0] is bwd[1]
    H.judge_all(f"p=0 separate={separate} {w}", H.forward_items(c, fwd, c.eps) + H.backward_items(c, fwd[0], fwd[2], fwd[3], bwd, c.depth), c.cls)


@pytest.mark.parametrize("w", WIDTHS)
def test_form_sinks(dev, w):
    with _form(dev, w) as c:
        fwd = _fwd(c)
        priors = tuple(H.small((w[0],), w[1], 310 + i, dev) for i in range(3))
        sinks = tuple(t.clone() for t in priors)
        bwd = _bwd(c, fwd[0], fwd[2], fwd[3], sinks=sinks)
    assert bwd[2] is None and bwd[3] is None and bwd[4] is None
    H.judge_all(f"sinks {w}", H.backward_items(c, fwd[0], fwd[2], fwd[3], bwd[:2] + sinks, c.depth, c.keep, P_B, priors=priors), c.cls)


# ---------------------------------------------------------------------------------------------- (C) alignment fallback
def _misaligned(t):
    """the same values at a storage offset of 4 elements: 8-byte aligned, not 16-byte aligned"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


@pytest.mark.parametrize("operand", ["x", "bias", "residual", "gamma", "beta"])
@pytest.mark.parametrize("cols", [768, 128])
def test_alignment_fallback_forward(dev, cols, operand):
    with _form(dev, (cols, BF16, 0)) as c:
        base = _fwd(c)
    for t in (c.x, c.bias, c.residual, c.gamma, c.beta):
        assert t.data_ptr() % 16 == 0
    with _family(2, 0):
        setattr(c, operand, _misaligned(getattr(c, operand)))
        out = _fwd(c)
    for name, a, b in zip(("z", "y", "mean", "rstd"), out, base):
        assert torch.equal(a, b), f"{name}: a misaligned {operand} did not take the one-wave-per-row kernel"
    H.judge_all(f"misaligned {operand} {cols}", H.forward_items(c, out, c.eps, c.keep, P_B), c.cls)


@pytest.mark.parametrize("operand", ["dy", "dz_in", "z", "gamma"])
@pytest.mark.parametrize("cols", [768, 128])
def test_alignment_fallback_backward(dev, cols, operand):
    with _form(dev, (cols, BF16, 0)) as c:
        z, _, mean, rstd = _fwd(c)
        base = _bwd(c, z, mean, rstd)
    with _family(2, 0):
        if operand == "z":
            z = _misaligned(z)
        else:
            setattr(c, operand, _misaligned(getattr(c, operand)))
        out = _bwd(c, z, mean, rstd)
    for name, a, b in zip(("dx", "dres", "dgamma", "dbeta", "dbias"), out, base):
        assert torch.equal(a, b), f"{name}: a misaligned {operand} did not take the one-wave-per-row kernel"
    H.judge_all(f"misaligned {operand} {cols}", H.backward_items(c, z, mean, rstd, out, H.bwd_depth(ROWS_B, cols, BF16, 2, aligned=False), c.keep, P_B), c.cls)


# ---------------------------------------------------------------------------------------------- (D) second / third trips round the grid-stride loops
def _big(name, cols, rows, variant=1, dtype=BF16):
    return pytest.param(dict(cols=cols, rows=rows, variant=variant, dtype=dtype), id=f"{name}-{cols}-{rows}")


# backward: 1024 workgroups of 4 * (rows per wave) rows. 384 columns reach the quarter-wave backward under variant 2 only.
BWD_BIG = [_big("wave", 100, 4101, 0), _big("wave", 100, 8195, 0), _big("wave-fp32", 768, 4101, dtype=F32), _big("half", 256, 8201, 2),
           _big("half", 768, 8201, 2), _big("half-lds", 768, 8201, 3), _big("quarter", 128, 16401), _big("quarter", 384, 16401, 2),
           _big("eighth", 192, 32801), _big("wide", 3072, 1027), _big("wide-fp32", 2052, 1027, dtype=F32)]
# forward: at most 8192 workgroups; the loads-first kernel is the DEFAULT from 65 536 rows of 768 columns (no force bit)
FWD_BIG = [_big("wave", 100, 32773, 0), _big("half", 256, 65545), _big("loads-first", 768, 65545), _big("quarter", 128, 131089),
           _big("eighth", 192, 262177), _big("wide-fp32", 2052, 8195, dtype=F32)]


def _big_case(dev, b, **make):
    rows, cols = b["rows"], b["cols"]
    p = 0.1 if rows * cols <= 4 << 20 else 0.0           # the host Philox restatement is the slow part
    c = H.make_case(rows, cols, b["dtype"], seed=400, device=dev, hard=False, **make)
    return c, p, H.keep_mask(SEED, OFFSET, rows, cols, p, dev), dict(p_drop=p, seed=SEED, offset=OFFSET)


@pytest.mark.parametrize("b", FWD_BIG)
def test_forward_second_pass(dev, b):
    from valor_amd import kernels as K
    t0 = time.perf_counter()
    c, p, keep, kw = _big_case(dev, b, dy=False, dz_in=False)
    gl = H.ln_group(b["cols"]) if (b["dtype"] == BF16 and b["variant"]) else 0
    groups = 1 if b["cols"] > 2048 else 4 * 64 // gl if gl else 4                          # rows per workgroup and trip
    assert H.FWD_BLOCKS_CAP * groups < b["rows"] <= 2 * H.FWD_BLOCKS_CAP * groups          # one full pass and a ragged handful
    with _family(b["variant"], 0):
        out = K.bdrln_fwd(c.x, c.bias, c.residual, c.gamma, c.beta, _eps(b["cols"]), **kw)
    try:
        H.judge_all(f"forward second pass {b}", H.forward_items(c, out, _eps(b["cols"]), keep, p))
    finally:
        torch.cuda.synchronize()
        print(f"DURATION forward {b['cols']} x {b['rows']}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("b", BWD_BIG)
def test_backward_second_pass(dev, b):
    from valor_amd import kernels as K
    t0 = time.perf_counter()
    c, p, keep, kw = _big_case(dev, b)
    rows, cols = b["rows"], b["cols"]
    z = c.residual                                      # the backward takes z, mean, rstd as inputs: benign rows and their fp64 statistics
    mean, rstd, *_ = H.ref_stats(z, _eps(cols))
    mean, rstd = mean.float(), rstd.float()
    with _family(b["variant"], 0):
        out = K.bdrln_bwd(c.dy, c.dz_in, z, mean, rstd, c.gamma, want_dbias=True, **kw)
    depth = H.bwd_depth(rows, cols, b["dtype"], b["variant"])
    assert depth > H.bwd_depth(37, cols, b["dtype"], b["variant"])                        # a second row group was taken
    try:
        H.judge_all(f"backward second pass {b}", H.backward_items(c, z, mean, rstd, out, depth, keep, p))
    finally:
        torch.cuda.synchronize()
        print(f"DURATION backward {cols} x {rows}: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------- (E) valor_colsum
@pytest.mark.parametrize("layout", ["contiguous", "slice-ld4", "slice-ld-odd"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_colsum_shapes(dev, dtype, layout):
    from valor_amd import kernels as K
    errs = []
    for rows in (1, 3, 4097, 5000):
        for cols in (4, 252, 255, 257, 3070):
            for start in ((0,) if layout == "contiguous" else (0, 8)):
                ld = cols if layout == "contiguous" else (cols + start + 11) // 4 * 4 + (0 if layout == "slice-ld4" else 1)
                buf = torch.full((rows, ld), float("nan"), dtype=dtype, device=dev)            # nothing outside the view may be read
                x = buf[:, start:start + cols]
                x.copy_(H.hard_rows(rows, cols, dtype, 500 + rows + cols, device=dev, hard=False))
                assert layout == "contiguous" or (ld % 4 == 0) == (layout == "slice-ld4")
                ref, mag = x.double().sum(0), x.double().abs().sum(0)
                depth = H.colsum_depth("colsum", rows)
                prior = H.small((cols,), dtype, 501, dev)
                got = K.colsum(x)
                acc = K.colsum(x, out=prior.clone(), accumulate=True)
                tag = f"colsum {layout} {dtype} {rows} x {cols} ld={ld} start={start}"
                try:
                    H.judge_all(tag, [("sum", got, ref, H.colsum_bound(mag, ref, depth, dtype)),
                                      ("accumulated", acc, ref + prior.double(), H.colsum_bound(mag, ref, depth, dtype, prior))])
                except AssertionError as e:
                    errs.append(str(e))
    assert not errs, "\n".join(errs[:8]) + f"\n({len(errs)} shapes failed)"


@pytest.mark.parametrize("nparts", [1024, 100, 7])
def test_colsum_finalize_fp32_output(dev, nparts):
    """valor_colsum_finalize called for bf16 tensors with out_f32 = 1: the sum of the fp32 partial rows is stored unrounded"""
    from valor_amd import kernels as K, lib
    cols = 257
    part = H.hard_rows(nparts, cols, F32, 600, device=dev, hard=False)
    prior = H.small((cols,), F32, 601, dev)
    ref, mag = part.double().sum(0), part.double().abs().sum(0)
    out, acc = torch.empty(cols, device=dev), prior.clone()
    lib.call("valor_colsum_finalize", K._stream(), lib.DT_BF16, part.data_ptr(), nparts, cols, out.data_ptr(), 1, 0)
    lib.call("valor_colsum_finalize", K._stream(), lib.DT_BF16, part.data_ptr(), nparts, cols, acc.data_ptr(), 1, 1)
    bound = (H.FIN_DEPTH + 1) * H.U32 * (mag + prior.double().abs())              # the finalize chain and the add onto the prior
    H.judge_all(f"finalize fp32 out nparts={nparts}", [("sum", out, ref, bound), ("accumulated", acc, ref + prior.double(), bound)])


# ---------------------------------------------------------------------------------------------- (F) refusals
def test_refusals(dev):
    from valor_amd import kernels as K, lib
    so = lib.load()
    st = K._stream()
    n = 8192
    buf = lambda dt=BF16: torch.full((n,), 7.0, dtype=dt, device=dev)
    x, bias, res, g, be, z, y, dy, dzi, dx, dres = (buf() for _ in range(11))
    mean, rstd, rsc, part = buf(F32), buf(F32), buf(F32), buf(F32)
    P = lambda t: t.data_ptr()

    def fwd(rows=2, cols=8, p=0.0, row_scale=0, rps=0):
        return so.valor_bdrln_fwd(st, lib.DT_BF16, P(x), P(bias), P(res), P(g), P(be), P(z), P(y), P(mean), P(rstd), rows, cols, 1e-5, p, 1, 0, row_scale, rps, 0)

    def bwd(rows=2, cols=8, dy_=None, dzi_=None, z_=None, row_scale=0, rps=0, dx_=None):
        ptr = lambda v, t: P(t) if v is None else v
        return so.valor_bdrln_bwd(st, lib.DT_BF16, ptr(dy_, dy), ptr(dzi_, dzi), ptr(z_, z), P(mean), P(rstd), P(g), ptr(dx_, dx), P(dres),
                                  0, 0, 0, rows, cols, 0.0, 1, 0, row_scale, rps, 0)

    assert fwd(cols=6) == ERR_ARG and bwd(cols=6) == ERR_ARG                   # cols % 4 != 0
    assert fwd(cols=4100) == ERR_ARG and bwd(cols=4100) == ERR_ARG            # cols > 4096
    assert fwd(p=1.0) == ERR_ARG
    assert fwd(row_scale=P(rsc), rps=0) == ERR_ARG and bwd(row_scale=P(rsc), rps=0) == ERR_ARG
    assert bwd(dy_=0, dzi_=0) == ERR_ARG                                       # neither dy nor dz_in
    assert bwd(z_=0) == ERR_ARG                                                # dy without z
    assert bwd(row_scale=P(rsc), rps=1, dx_=P(dres)) == ERR_ARG               # a row scale needs its own dx
    assert fwd(rows=0) == 0 and bwd(rows=0) == 0
    torch.cuda.synchronize()
    for t in (z, y, mean, rstd, dx, dres, part):
        assert (t == 7.0).all()
