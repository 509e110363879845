"""The fused bias + dropout + residual + LayerNorm kernels (csrc/layernorm.hip) WITH dropout, every family, against the Philox keep mask
restated on the host (tests/dropout_ref.py ln_keep: counter offset + (row * cols + c) / 4, word c % 4):
 (a) exact mask -- x = 1, no bias, residual = 0: (z != 0) is the host mask element for element (on rows whose stochastic-depth scale is
     non-zero), and the backward's (dx != 0) for dz_in = 1 is the same mask;
 (b) fp64 parity on random inputs with that mask: z, y, mean, rstd, dx, dres, dgamma, dbeta, dbias at the tolerances of
     test_gemm_ln_gpu.py::test_bdrln_fwd_bwd (fp32: 3e-6 forward, 2e-5 backward; bf16: 8e-3 / 2e-2).
Families are chosen through valor_ln_set_variant / valor_ln_set_nt (launch_ln_fwd / launch_ln_bwd); rows 37 and 333 are odd, so the
last workgroup's lane groups are left without a row."""
import contextlib

import pytest
import torch

import dropout_ref as R
from test_gemm_ln_gpu import _mk, _rel

pytestmark = pytest.mark.gpu
DEVICE_BASE = 3 * 2 ** 40 + 12345
BF16, F32 = torch.bfloat16, torch.float32


@contextlib.contextmanager
def _family(variant, nt):
    from valor_amd import lib
    so = lib.load()
    old_v, old_n = so.valor_ln_set_variant(-1), so.valor_ln_set_nt(-1)
    try:
        so.valor_ln_set_variant(variant)
        so.valor_ln_set_nt(nt)
        yield
    finally:
        so.valor_ln_set_variant(old_v)
        so.valor_ln_set_nt(old_n)


def _case(name, cols, variant=1, nt=0, dtype=BF16, p=0.1, scaled=False, base=0):
    return pytest.param(dict(cols=cols, variant=variant, nt=nt, dtype=dtype, p=p, scaled=scaled, base=base), id=f"{name}-{cols}")


CASES = (
    # variant 0: ln_fwd_kernel / ln_bwd_kernel, one wave per row (1280 columns: NV = 6 with dead vector slots)
    [_case("wave", c, variant=0) for c in (100, 768, 1280, 2048)]
    # variant 1 (default): ln_fwd_h_kernel on half / quarter / eighth of a wave, ln_bwd_h_kernel at <= 256 and 1024 columns, ln_bwd_kernel else
    + [_case("default", c, variant=1) for c in (128, 192, 256, 384, 512, 768, 1024)]
    # variant 2: ln_bwd_h_kernel everywhere
    + [_case("half", c, variant=2) for c in (128, 192, 256, 384, 512, 768, 1024)]
    + [_case("lds-accumulators", 768, variant=3),            # ln_bwd_h_kernel<3, 32, true>
       _case("loads-first", 768, nt=64),                     # ln_fwd_h2_kernel<3, 1>
       _case("non-temporal", 768, nt=31),                    # nt bits 0-4: x loads, y / z stores, backward loads and stores
       _case("wide", 3072),                                  # ln_fwd_wide_kernel / ln_bwd_wide_kernel (4 waves per row)
       _case("wide-fp32", 2052, dtype=F32),
       _case("fp32", 768, dtype=F32),
       _case("row-scale", 768, scaled=True),                 # stochastic depth: rows_per_scale = 7, some scales zero
       _case("row-scale-wave", 100, variant=0, scaled=True),
       _case("p0.25", 768, p=0.25),
       _case("device-base", 768, base=DEVICE_BASE)])
SEED, OFFSET, RPS = 7, 11, 7


@pytest.fixture
def device_rng(dev):
    from valor_amd import ops
    ops.DropoutState.disable_device_base()
    yield ops.DropoutState
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)


@contextlib.contextmanager
def _setup(dev, device_rng, c):
    with _family(c["variant"], c["nt"]):
        if c["base"]:
            device_rng.enable_device_base(dev).fill_(c["base"])
        try:
            yield
        finally:
            device_rng.disable_device_base()


def _row_scale(rows, dev):
    n = (rows + RPS - 1) // RPS
    vals = torch.tensor([1.25, 0.0, 1.25, 0.5, 0.0, 2.0])
    return vals[torch.arange(n) % len(vals)].to(dev)


def _keep(dev, c, rows):
    return torch.from_numpy(R.ln_keep(SEED, OFFSET + c["base"], rows, c["cols"], c["p"])).to(dev)


@pytest.mark.parametrize("rows", [37, 333])
@pytest.mark.parametrize("c", CASES)
def test_exact_mask(dev, device_rng, c, rows):
    from valor_amd import kernels as K
    cols, p, dtype = c["cols"], c["p"], c["dtype"]
    rs = _row_scale(rows, dev) if c["scaled"] else None
    kw = dict(p_drop=p, seed=SEED, offset=OFFSET, row_scale=rs, rows_per_scale=RPS if c["scaled"] else 0)
    x = torch.ones((rows, cols), dtype=dtype, device=dev)
    with _setup(dev, device_rng, c):
        z, _, _, _ = K.bdrln_fwd(x, None, torch.zeros_like(x), None, None, 1e-5, **kw)
        dx, dres, *_ = K.bdrln_bwd(None, torch.ones_like(x), None, None, None, None, want_dgamma=False, want_dbeta=False, **kw)
    keep = _keep(dev, c, rows)
    live = torch.ones(rows, dtype=torch.bool, device=dev)
    if rs is not None:
        live = rs[torch.arange(rows, device=dev) // RPS] != 0
        assert (z[~live] == 0).all() and (dx[~live] == 0).all() and 0 < int(live.sum()) < rows
    assert torch.equal((z != 0)[live], keep[live])
    assert torch.equal((dx != 0)[live], keep[live])
    assert torch.equal(dres, torch.ones_like(x))
    scale = torch.ones(rows, device=dev) if rs is None else rs[torch.arange(rows, device=dev) // RPS]
    want = keep.double() * R.keep_scale(p) * scale.double()[:, None]           # and the kept values, to the rounding of the storage type
    rtol = 1e-6 if dtype == torch.float32 else 2.0 ** -8
    assert torch.allclose(z.double(), want, rtol=rtol, atol=0) and torch.allclose(dx.double(), want, rtol=rtol, atol=0)


@pytest.mark.parametrize("rows", [37, 333])
@pytest.mark.parametrize("c", CASES)
def test_fp64_parity(dev, device_rng, c, rows):
    from valor_amd import kernels as K
    cols, p, dtype = c["cols"], c["p"], c["dtype"]
    rs = _row_scale(rows, dev) if c["scaled"] else None
    kw = dict(p_drop=p, seed=SEED, offset=OFFSET, row_scale=rs, rows_per_scale=RPS if c["scaled"] else 0)
    x = _mk((rows, cols), dtype, dev, 1); bias = _mk((cols,), dtype, dev, 2); res = _mk((rows, cols), dtype, dev, 3)
    g = _mk((cols,), dtype, dev, 4) + 1.0; be = _mk((cols,), dtype, dev, 5)
    dy = _mk((rows, cols), dtype, dev, 6); dzin = _mk((rows, cols), dtype, dev, 7)
    eps = 1e-12 if cols == 768 else 1e-5
    with _setup(dev, device_rng, c):
        z, y, mean, rstd = K.bdrln_fwd(x, bias, res, g, be, eps, **kw)
        dx, dres, dg, db, dbias = K.bdrln_bwd(dy, dzin, z, mean, rstd, g, want_dbias=True, **kw)
    xd, bd, rd, gd, bed = [t.double().requires_grad_(True) for t in (x, bias, res, g, be)]
    zr, yr = R.ref_bdrln_dropout(xd, bd, rd, gd, bed, eps, _keep(dev, c, rows), p, rs, RPS)
    ((yr * dy.double()).sum() + (zr * dzin.double()).sum()).backward()
    zr = zr.detach()
    var = zr.var(-1, unbiased=False)
    tol_f, tol_b = (3e-6, 2e-5) if dtype == torch.float32 else (8e-3, 2e-2)
    fwd = {"z": _rel(z, zr), "y": _rel(y, yr.detach()), "mean": _rel(mean, zr.mean(-1)), "rstd": _rel(rstd, (var + eps).rsqrt())}
    bwd = {"dx": _rel(dx, xd.grad), "dres": _rel(dres, rd.grad), "dgamma": _rel(dg, gd.grad), "dbeta": _rel(db, bed.grad), "dbias": _rel(dbias, bd.grad)}
    print("PARITY ln", c, rows, {n: f"{e:.2e}" for n, e in {**fwd, **bwd}.items()}, f"tol {tol_f:g}/{tol_b:g}")
    assert dx.data_ptr() != dres.data_ptr()
    for n, e in fwd.items():
        assert e < tol_f, (n, e)
    for n, e in bwd.items():
        assert e < tol_b, (n, e)
