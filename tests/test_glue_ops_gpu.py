"""The small kernels of misc.hip that sit between the GEMMs (patchify, frame / type add, L2 normalise, row gather / scatter / tap, row
dot, dact_mul, the fp32 cast) and the two fp32 means, each against an fp64 torch reference built from the ROUNDED inputs, at the smallest
shapes that cross a boundary of the kernel: 4 elements per lane x 64 lanes = 256 columns per pass, 4 rows (waves) per block, and the
grid cap of 8192 blocks x 256 threads = 2 097 152 work items, above which the grid-stride loop makes a second pass.

Tolerances are elementwise and come from the arithmetic (U32 = 2^-24, the half-ulp of fp32; U(dtype) the half-ulp of the output type):
one rounding to the output type costs U(dtype) * |ref|, a sum of n terms accumulated in fp32 costs n * U32 * sum |term_i|, and every
comparison allows twice the bound so derived (_close). Pure data movement is compared bit for bit (_same_bits)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
GRID_ITEMS = 8192 * 256            # grid_for(): the work items one pass of a capped grid covers
DTYPES = [torch.float32, torch.bfloat16]


def U(dtype):
    return 2.0 ** -9 if dtype == torch.bfloat16 else U32


def _once(ref, dtype):
    """bound of ONE fp32 operation whose result is stored as dtype: fp32 rounds once; bf16 rounds the fp32 result a second time"""
    return ref.abs() * (U(dtype) + (U32 if dtype == torch.bfloat16 else 0.0))


def _close(got, ref, bound, what=""):
    """elementwise |got - ref| <= 2 * bound (a NaN on either side fails)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = (bound.detach().double().cpu() if torch.is_tensor(bound) else torch.tensor(float(bound), dtype=torch.float64)).expand_as(ref)
    err = (got - ref).abs()
    ok = err <= 2.0 * bound
    if not bool(ok.all()):
        i = int((~ok).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements off, first at flat index {i}: got {got.flatten()[i]!r} "
                             f"want {ref.flatten()[i]!r} allowed {2.0 * bound.flatten()[i]!r}")


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = _bits(got), _bits(want)
    if not torch.equal(a, b):
        i = int((a != b).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, first at flat index {i}: "
                             f"{got.flatten()[i].item()!r} vs {want.flatten()[i].item()!r}")


def _randn(g, shape, dtype, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).to(dtype)


def _call(name, *args):
    from valor_amd import lib
    return lib.call(name, *args)


def _kp():
    from valor_amd.kernels import _ptr, _stream, dt_of
    return _ptr, _stream, dt_of


# ------------------------------------------------------------------------------------------------ L2 normalise
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5, 1003])
@pytest.mark.parametrize("cols", [4, 252, 256, 260, 768])
def test_l2_normalize(dev, dtype, rows, cols):
    """ops.l2_normalize forward, the saved fp32 norm and the backward against x / x.norm().clamp_min(1e-12) in fp64 under autograd.
    cols: one busy lane, just under / exactly / just over one 256-column pass, three passes; rows: one wave, a second block with three
    idle waves, 251 blocks with one idle wave. With rows >= 5, row 1 is all zero (the 1e-12 clamp: y = 0, dx = dy / 1e-12) and row 3 is
    scaled by 1e15 (squares ~1e30, their sum far beyond what fp32 holds exactly, a factor 1e5 short of overflow)."""
    from valor_amd import ops
    _ptr, _stream, dt_of = _kp()
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x0 = torch.randn((rows, cols), generator=g)
    if rows >= 5:
        x0[1] = 0.0
        x0[3] *= 1e15
    x0 = x0.to(dtype)
    dy0 = _randn(g, (rows, cols), dtype)            # |dy| ~ 1: the zero row's gradient dy * 1e12 stays finite in bf16 and fp32
    x = x0.to(dev).requires_grad_(True)
    y = ops.l2_normalize(x)
    y.backward(dy0.to(dev))
    # the same through lib.call (the fp32 norm vector is visible there), on buffers that own ONE GUARD ROW behind the last: a wave that
    # takes row == rows (the first idle wave of the last block) would write it
    guard = lambda t, v: torch.cat((t, torch.full((1,) + tuple(t.shape[1:]), v, dtype=t.dtype))).to(dev)
    xg, dyg = guard(x0, 1.0), guard(dy0, 1.0)
    y2 = torch.full((rows + 1, cols), 7.0, dtype=dtype, device=dev)
    dx2 = torch.full((rows + 1, cols), 7.0, dtype=dtype, device=dev)
    norm = torch.full((rows + 1,), 7.0, dtype=torch.float32, device=dev)
    _call("valor_l2norm_fwd", _stream(), dt_of(y2), _ptr(xg), _ptr(y2), _ptr(norm), rows, cols)
    _call("valor_l2norm_bwd", _stream(), dt_of(y2), _ptr(y2), _ptr(dyg), _ptr(norm), _ptr(dx2), rows, cols)
    torch.cuda.synchronize()
    norm, ng = norm[:rows], norm[rows:]

    xr = x0.double().requires_grad_(True)
    nr = xr.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    yr = xr / nr
    yr.backward(dy0.double())
    yr, nr = yr.detach(), nr.detach()
    # norm = sqrt(sum of cols squares): the products round once each, the sum accumulates cols terms -> relative (cols + 1) U32 on the
    # sum, half of it on the root, + U32 for sqrtf itself (correctly rounded); the clamp constant 1e-12f is within U32 of 1e-12
    e_n = ((cols + 1) / 2 + 1) * U32
    _close(norm, nr[:, 0], nr[:, 0] * e_n, "norm")
    # y = x * (1 / norm): + one division, one product (U32 each), one rounding to the output type
    e_y = e_n + 2 * U32 + U(dtype)
    _close(y, yr, yr.abs() * e_y, "y")
    _same_bits(y2, guard(y.detach().cpu(), 7.0), "y through lib.call, guard row untouched")
    assert float(ng) == 7.0, "norm[rows] untouched"
    # dx = (dy - y s) / norm with the STORED y (relative error e_y) and s = <y, dy> (cols terms in fp32, each carrying y's error):
    #   |s' - s| <= (e_y + (cols + 1) U32) sum |y dy| =: ds;   |y' s' - y s| <= |y| ds + |y s| (e_y + U32), the subtraction rounds once
    #   more (U32 (|dy| + |y s|)); the quotient carries the norm's error, the division and product (U32 each) and the output rounding
    dyr = dy0.double()
    s = (yr * dyr).sum(-1, keepdim=True)
    ds = (e_y + (cols + 1) * U32) * (yr * dyr).abs().sum(-1, keepdim=True)
    num = yr.abs() * ds + (yr * s).abs() * (e_y + 2 * U32) + dyr.abs() * U32
    b_dx = num / nr + xr.grad.abs() * (e_n + 2 * U32 + U(dtype))
    _close(x.grad, xr.grad, b_dx, "dx")
    _same_bits(dx2, guard(x.grad.cpu(), 7.0), "dx through lib.call, guard row untouched")
    if rows >= 5:
        assert float(y[1].float().abs().max()) == 0.0 and bool(torch.isfinite(x.grad.float()).all())


# ------------------------------------------------------------------------------------------------ row dot
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (1, 17), (8, 125)])
@pytest.mark.parametrize("cols", [4, 256, 260, 768])
def test_rowdot(dev, dtype, bias, B, T, cols):
    """ops.rowdot (Linear(E -> 1)) y, dx, dw, db on a [B, T, E] input. cols 260: a second workgroup of rowdot_bwd_dw_kernel in which only
    lane 0 has columns; rows 1 / 15 / 17 / 1000: the 16-way row split with empty groups, a short one, exactly one row over, many. Without
    a bias the kernel gets db = null."""
    from valor_amd import ops
    rows = B * T
    g = torch.Generator().manual_seed(rows * 7 + cols)
    x0, w0, dy0 = _randn(g, (B, T, cols), dtype), _randn(g, (1, cols), dtype), _randn(g, (B, T, 1), dtype)
    b0 = _randn(g, (1,), dtype) if bias else None
    x, w = x0.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True)
    b = b0.to(dev).requires_grad_(True) if bias else None
    y = ops.rowdot(x, w, b)
    assert y.shape == (B, T, 1)
    y.backward(dy0.to(dev))
    torch.cuda.synchronize()

    xr, wr = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    br = b0.double().requires_grad_(True) if bias else None
    yr = (xr * wr[0]).sum(-1, keepdim=True) + (br if bias else 0.0)
    yr.backward(dy0.double())
    yr = yr.detach()
    # cols products summed in fp32 (+ the bias: one more term), then one rounding to the output type
    mag = (xr.detach() * wr.detach()[0]).abs().sum(-1, keepdim=True) + (b0.double().abs() if bias else 0.0)
    _close(y, yr, (cols + 2) * U32 * mag + U(dtype) * yr.abs(), "y")
    _close(x.grad, xr.grad, _once(xr.grad, dtype), "dx")                   # dx[m, k] = dy[m] w[k]: one product
    # dw[k] = sum_m dy[m] x[m, k]: rows products, split 16 ways and the 16 partials added: at most rows + 16 additions on any path
    n = rows + 17
    magw = (dy0.double() * x0.double()).abs().sum((0, 1))
    _close(w.grad, wr.grad, n * U32 * magw[None] + U(dtype) * wr.grad.abs(), "dw")
    if bias:
        _close(b.grad, br.grad, n * U32 * dy0.double().abs().sum() + U(dtype) * br.grad.abs(), "db")


# ------------------------------------------------------------------------------------------------ frame / type add
def _frame_type_ref(x0, fe0, te0):
    """x [b, F, X, E] + frame_emb[:F] (a table with MORE rows than frames) + type_emb, flattened to [b, F*X, E]; fp64 leaves"""
    xr, fr, tr = (t.double().requires_grad_(True) for t in (x0, fe0, te0))
    b, Fn, X, E = x0.shape
    out = (xr + fr[:Fn][None, :, None, :] + tr).reshape(b, Fn * X, E)
    mag = (xr.detach().abs() + fr.detach()[:Fn][None, :, None, :].abs() + tr.detach().abs()).reshape(b, Fn * X, E)
    return xr, fr, tr, out, mag


def _check_frame_type_grads(dtype, got, leaves, dslice, Fn, what):
    """got = (dx, dframe, dtype_emb) of the kernel; leaves = the fp64 leaves after backward; dslice = this modality's rows of dout"""
    dx, dfe, dte = got
    xr, fr, tr = leaves
    b, _, X, E = xr.shape
    _same_bits(dx, dslice.reshape(xr.shape), what + " din (a copy of the dout slice)")
    # dframe[f] = sum over the b * X (sample, token) pairs: 64 slices x 4 waves stride over them, 4 + 64 partials are added in fp32,
    # one rounding to the output type
    n = b * X + 68
    d4 = dslice.double().cpu().reshape(b, Fn, X, E)
    b_f = n * U32 * d4.abs().sum((0, 2)) + U(dtype) * fr.grad[:Fn].abs()
    _close(dfe[:Fn], fr.grad[:Fn], b_f, what + " dframe")
    assert float(dfe[Fn:].float().abs().max()) == 0.0, what + ": rows of the frame table beyond F carry no gradient"
    assert float(fr.grad[Fn:].abs().max()) == 0.0
    # dtype = column sums of the STORED dframe[:F] (each carrying its own error b_f), F terms in fp32, one rounding
    b_t = b_f.sum(0) + (Fn + 1) * U32 * fr.grad[:Fn].abs().sum(0) + U(dtype) * tr.grad.abs()
    _close(dte, tr.grad, b_t, what + " dtype")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [4, 256, 260, 768])
@pytest.mark.parametrize("b,Fn,X,A,Y", [(1, 3, 1, 2, 257), (5, 2, 51, 3, 140)])
def test_cross_input(dev, dtype, E, b, Fn, X, A, Y):
    """ops.cross_input: [video + frame + type | audio + frame + type] and all six gradients. b * X / b * Y = 1, 257, 255, 700 pairs
    against the 256-way split of frame_sum_partial_kernel; F != A and X != Y, so the audio half's row offset F * X is not A * Y; both
    frame tables have more rows than frames. Each forward launch must leave the OTHER modality's bytes of `out` alone."""
    from valor_amd import ops
    _ptr, _stream, dt_of = _kp()
    g = torch.Generator().manual_seed(E + b)
    v0, a0 = _randn(g, (b, Fn, X, E), dtype), _randn(g, (b, A, Y, E), dtype)
    vf0, af0 = _randn(g, (Fn + 3, E), dtype), _randn(g, (A + 2, E), dtype)
    vt0, at0 = _randn(g, (E,), dtype), _randn(g, (E,), dtype)
    Sv, Sa = Fn * X, A * Y
    dout0 = _randn(g, (b, Sv + Sa, E), dtype)
    leaves = [t.to(dev).requires_grad_(True) for t in (v0, a0, vf0, vt0, af0, at0)]
    out = ops.cross_input(*leaves)
    out.backward(dout0.to(dev))
    torch.cuda.synchronize()

    vr, vfr, vtr, outv, magv = _frame_type_ref(v0, vf0, vt0)
    ar, afr, atr, outa, maga = _frame_type_ref(a0, af0, at0)
    ref = torch.cat((outv, outa), dim=1)
    ref.backward(dout0.double())
    # two fp32 additions, one rounding to the output type
    bound = 2 * U32 * torch.cat((magv, maga), dim=1) + U(dtype) * ref.detach().abs()
    _close(out, ref, bound, "out")
    v, a, vf, vt, af, at = leaves
    _check_frame_type_grads(dtype, (v.grad, vf.grad, vt.grad), (vr, vfr, vtr), dout0[:, :Sv], Fn, "video")
    _check_frame_type_grads(dtype, (a.grad, af.grad, at.grad), (ar, afr, atr), dout0[:, Sv:], A, "audio")

    # one forward launch at a time into a NaN-filled buffer: its own rows equal what ops produced, the other modality's stay NaN
    nan = torch.full((b, Sv + Sa, E), float("nan"), dtype=dtype, device=dev)
    for x_, fe, te, Fq, Xq, off, mine in ((v, vf, vt, Fn, X, 0, slice(0, Sv)), (a, af, at, A, Y, Sv, slice(Sv, Sv + Sa))):
        buf = nan.clone()
        _call("valor_add_frame_type_fwd", _stream(), dt_of(buf), _ptr(x_.detach()), _ptr(fe.detach()), _ptr(te.detach()), _ptr(buf),
              b, Fq, Xq, E, (Sv + Sa) * E, off)
        want = nan.clone()
        want[:, mine] = out.detach()[:, mine]
        _same_bits(buf, want, f"forward at row offset {off}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [4, 256, 260, 768])
@pytest.mark.parametrize("b,Fn,X", [(1, 3, 1), (15, 2, 17), (257, 3, 1), (7, 2, 100)])
def test_single_input(dev, dtype, E, b, Fn, X):
    """ops.single_input (one modality) and its three gradients; b * X = 1, 255, 257, 700 pairs"""
    from valor_amd import ops
    g = torch.Generator().manual_seed(E + b)
    x0, fe0, te0 = _randn(g, (b, Fn, X, E), dtype), _randn(g, (Fn + 2, E), dtype), _randn(g, (E,), dtype)
    dout0 = _randn(g, (b, Fn * X, E), dtype)
    x, fe, te = (t.to(dev).requires_grad_(True) for t in (x0, fe0, te0))
    out = ops.single_input(x, fe, te)
    out.backward(dout0.to(dev))
    torch.cuda.synchronize()
    xr, fr, tr, ref, mag = _frame_type_ref(x0, fe0, te0)
    ref.backward(dout0.double())
    _close(out, ref, 2 * U32 * mag + U(dtype) * ref.detach().abs(), "out")       # two fp32 additions, one rounding
    _check_frame_type_grads(dtype, (x.grad, fe.grad, te.grad), (xr, fr, tr), dout0, Fn, "single")


# ------------------------------------------------------------------------------------------------ gather / scatter / tap
def _gather_ref(x0, idx):
    """x0[idx] with a zero row wherever idx < 0 (data movement: same dtype)"""
    out = x0[idx.clamp_min(0)].clone()
    out[idx < 0] = 0
    return out


def _scatter_ref(shape, idx, d0):
    dx = torch.zeros(shape, dtype=d0.dtype)
    dx[idx[idx >= 0]] = d0[idx >= 0]
    return dx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,n,E", [(9, 7, 4), (40, 23, 260), (13000, 12000, 768)])
def test_gather_rows(dev, dtype, R, n, E):
    """ops.gather_rows: negative indices give zero rows forward and dropped gradients backward; repeated valid indices forward only
    (scatter's contract is unique indices). n = 12 000 rows of 768: 2 304 000 four-element items, a second grid-stride pass of both
    kernels. All of it is data movement: bit for bit."""
    from valor_amd import ops
    g = torch.Generator().manual_seed(n)
    x0, d0 = _randn(g, (R, E), dtype), _randn(g, (n, E), dtype)
    idx = torch.randperm(R, generator=g)[:n]
    idx[torch.randperm(n, generator=g)[:max(2, n // 10)]] = -1
    idx[0] = -1
    rep = idx.clone()
    rep[1] = rep[2] = rep[n - 2] = idx[idx >= 0][0]
    with torch.no_grad():
        _same_bits(ops.gather_rows(x0.to(dev), rep.to(dev)), _gather_ref(x0, rep), "forward with repeated indices")
    x = x0.to(dev).requires_grad_(True)
    out = ops.gather_rows(x, idx.to(dev))
    out.backward(d0.to(dev))
    torch.cuda.synchronize()
    _same_bits(out.detach(), _gather_ref(x0, idx), "forward")
    _same_bits(x.grad, _scatter_ref((R, E), idx, d0), "backward")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_scatter_column_slice(dev, dtype):
    """valor_gather_rows / valor_scatter_rows on a column slice of a wider matrix (src_ld / dst_ld > E), which ops never passes: the
    gather reads only the slice's columns, the scatter leaves every column outside the slice and every row not named alone (NaN-filled),
    the guard row in FRONT of the destination included: that is where an index of -1 would land if it were not dropped"""
    _ptr, _stream, dt_of = _kp()
    R, n, E, ld, c0 = 21, 9, 260, 272, 8
    g = torch.Generator().manual_seed(5)
    wide0 = _randn(g, (R, ld), dtype)
    idx = torch.randperm(R, generator=g)[:n]
    idx[4] = -1
    wide, idx_d = wide0.to(dev), idx.to(dev)
    out = torch.empty((n, E), dtype=dtype, device=dev)
    _call("valor_gather_rows", _stream(), dt_of(out), _ptr(wide[:, c0:]), _ptr(idx_d), _ptr(out), n, E, ld)
    _same_bits(out, _gather_ref(wide0[:, c0:c0 + E], idx), "gather from a column slice")
    src0 = _randn(g, (n, E), dtype)
    big = torch.full((R + 1, ld), float("nan"), dtype=dtype, device=dev)
    src_d = src0.to(dev)
    _call("valor_scatter_rows", _stream(), dt_of(big), _ptr(src_d), _ptr(idx_d), _ptr(big[1:, c0:]), n, E, ld)
    want = torch.full((R + 1, ld), float("nan"), dtype=dtype)
    want[idx[idx >= 0] + 1, c0:c0 + E] = src0[idx >= 0]
    _same_bits(big, want, "scatter into a column slice")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use", ["both", "rows", "through"])
def test_tap_rows(dev, dtype, use, monkeypatch):
    """ops.tap_rows with FUSE_GLUE on: (x, x[idx]) as one node. Its gradient must be that of x and x[idx] taken separately (fp64
    autograd): with both outputs used the tapped rows hold ONE addition of two values of the output type (one rounding), every other row
    is the pass-through gradient bit for bit; with one output used it is data movement. In fp32 the unfused route (FUSE_GLUE off:
    autograd adds the two gradients) performs the same single fp32 addition: bit-identical."""
    from valor_amd import ops
    monkeypatch.setattr(ops, "FUSE_GLUE", True)
    R, n, E = 37, 11, 260
    g = torch.Generator().manual_seed(R)
    x0, dA0, dB0 = _randn(g, (R, E), dtype), _randn(g, (R, E), dtype), _randn(g, (n, E), dtype)
    idx = torch.randperm(R, generator=g)[:n]

    def run():
        x = x0.to(dev).requires_grad_(True)
        thru, rows = ops.tap_rows(x, idx.to(dev))
        _same_bits(thru.detach(), x0, "pass-through")
        _same_bits(rows.detach(), x0[idx], "tapped rows")
        outs, grads = [], []
        if use in ("both", "through"):
            outs.append(thru); grads.append(dA0.to(dev).clone())         # (the node updates this gradient in place)
        if use in ("both", "rows"):
            outs.append(rows); grads.append(dB0.to(dev).clone())
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
        return x.grad

    got = run()
    xr = x0.double().requires_grad_(True)
    loss = 0.0
    if use in ("both", "through"):
        loss = loss + (xr * dA0.double()).sum()
    if use in ("both", "rows"):
        loss = loss + (xr[idx] * dB0.double()).sum()
    loss.backward()
    if use == "both":
        _close(got, xr.grad, xr.grad.abs() * U(dtype), "dx")              # one addition, rounded once to the output type
        rest = torch.ones(R, dtype=torch.bool); rest[idx] = False
        _same_bits(got[rest.to(dev)], dA0[rest], "rows that were not tapped")
    else:
        _same_bits(got, xr.grad.to(dtype), "dx")
    if dtype == torch.float32:
        monkeypatch.setattr(ops, "FUSE_GLUE", False)
        _same_bits(run(), got, "FUSE_GLUE off")


# ------------------------------------------------------------------------------------------------ patchify
def _patch_rows(img, P):
    """nn.Conv2d(kernel = stride = P) as rows: F.unfold gives [N, C*P*P, L] in the conv weight's (c, i, j) order"""
    K = img.shape[1] * P * P
    return F.unfold(img.double(), kernel_size=P, stride=P).transpose(1, 2).reshape(-1, K)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,C,H,W,P,pad_to", [(2, 3, 32, 48, 16, 0), (3, 1, 64, 32, 16, 0), (2, 3, 28, 42, 14, 592), (1821, 3, 32, 48, 16, 0)])
def test_patchify(dev, dtype, N, C, H, W, P, pad_to):
    """ops.patchify against F.unfold: CLIP B/16 (4 pixels per thread), AST (one channel, non-square), ViT-L/14 (2 pixels per thread, rows
    padded 588 -> 592 with zeros the kernel must not touch), and N = 1821 images: 2 097 792 items, one past the grid cap. fp32 output is
    a copy, bf16 output is the round-to-nearest-even of it: bit for bit."""
    from valor_amd import ops
    g = torch.Generator().manual_seed(N + P)
    img = torch.randn((N, C, H, W), generator=g)
    if N > 1000:
        assert N * C * H * W // 4 > GRID_ITEMS >= (N - 1) * C * H * W // 4
    out = ops.patchify(img.to(dev), P, dtype, pad_to=pad_to)
    K = C * P * P
    assert out.shape == (N * (H // P) * (W // P), max(K, pad_to))
    _same_bits(out[:, :K], _patch_rows(img, P).to(torch.float32).to(dtype), "patch rows")
    if pad_to:
        assert float(out[:, K:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_patchify_unaligned_row_stride(dev, dtype):
    """valor_patchify with ld_out = K + 2 at P = 16: a row stride that is no multiple of 4 elements forces the 2-pixel path on a patch
    size that otherwise takes the 4-pixel one; the two pad columns stay as they were (NaN)"""
    _ptr, _stream, dt_of = _kp()
    N, C, H, W, P = 2, 3, 32, 48, 16
    K = C * P * P
    g = torch.Generator().manual_seed(3)
    img = torch.randn((N, C, H, W), generator=g)
    rows = N * (H // P) * (W // P)
    out = torch.full((rows, K + 2), float("nan"), dtype=dtype, device=dev)
    _call("valor_patchify", _stream(), dt_of(out), _ptr(img.to(dev)), _ptr(out), N, C, H, W, P, K + 2)
    want = torch.full((rows, K + 2), float("nan"), dtype=dtype)
    want[:, :K] = _patch_rows(img, P).to(torch.float32).to(dtype)
    _same_bits(out, want, "rows of K + 2 columns")


# ------------------------------------------------------------------------------------------------ dact_mul
ACTS = {"gelu_erf": 1, "quick_gelu": 2, "relu": 3, "tanh": 4}
# max |act'(u) evaluated by torch in fp32 on the CPU - the same formula in fp64| over ALL the values _dact_inputs draws (fp32 inputs, the
# three sizes pooled: the four-element case alone holds only 0 and +-1e-30, where torch is exact and says nothing about another
# implementation). Measured on the CPU, see test_dact_mul's docstring. The kernel may use another few-ulp implementation: 8 x is allowed.
DACT_FP32_ERR = {"gelu_erf": 1.44e-7, "quick_gelu": 8.45e-7, "relu": 0.0, "tanh": 9.1e-8}


def _dact(u, act):
    """act'(u), the formulas of act_bwd_c (common.h) in u's own precision"""
    if act == "gelu_erf":          # Phi(u) + u phi(u)
        return 0.5 * (1.0 + torch.erf(u * 0.7071067811865476)) + u * 0.3989422804014327 * torch.exp(-0.5 * u * u)
    if act == "quick_gelu":        # s + 1.702 u s (1 - s), s = sigmoid(1.702 u)
        s = torch.sigmoid(1.702 * u)
        return s + 1.702 * u * s * (1.0 - s)
    if act == "relu":              # u > 0 ? 1 : 0 -- the derivative AT zero is 0
        return (u > 0).to(u.dtype)
    t = torch.tanh(u)
    return 1.0 - t * t


def _dact_inputs(n, dtype, seed=11):
    g = torch.Generator().manual_seed(seed)
    u = 2.0 * torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 3.0, -3.0, 10.0, -10.0, 40.0, -40.0])
    k = min(n, special.numel())
    u[:k] = special[:k]
    if n > 2 * special.numel():
        u[-special.numel():] = special          # the tail too: the last items of the last grid-stride pass
    dh = torch.randn(n, generator=g)
    return dh.to(dtype), u.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [4, 1020, GRID_ITEMS * 4 + 4])
@pytest.mark.parametrize("act", sorted(ACTS))
def test_dact_mul(dev, dtype, act, n):
    """valor_dact_mul: du = dh * act'(u) for the four activations; u holds 0, -0, +-1e-30, +-{1, 3, 10, 40} (the saturated tails, ReLU at
    and around 0) besides 2 N(0, 1); n = one thread, four blocks with a partial last one, one item past the grid cap.
    The device evaluates act' with hardware exp / rcp and a polynomial erf, whose error is not derivable from roundings: measured
    instead, the same formulas in torch fp32 on the CPU against fp64 on these inputs differ by at most (n = 1020 / n = 8 388 612; 0 at
    n = 4) 1.05e-7 / 1.44e-7 (gelu_erf), 6.50e-7 / 8.44e-7 (quick_gelu: 1 - s cancels for large u), 8.2e-8 / 9.05e-8 (tanh) and 0 (relu);
    the kernel gets 8 x the maximum, i.e. 1.15e-6 / 6.76e-6 / 7.3e-7 / 0 absolute on act', times |dh|, plus the product's and the output's
    rounding. ReLU'(0) is 0 (act_bwd_c: x > 0 ? 1 : 0)."""
    _ptr, _stream, dt_of = _kp()
    dh0, u0 = _dact_inputs(n, dtype)
    dh, u = dh0.to(dev), u0.to(dev)
    du = torch.empty_like(dh)
    _call("valor_dact_mul", _stream(), dt_of(dh), _ptr(dh), _ptr(u), _ptr(du), n, ACTS[act])
    torch.cuda.synchronize()
    d = _dact(u.double(), act)                      # fp64 on the device: eight million values per case
    ref = dh.double() * d
    _close(du, ref, dh.double().abs() * 8.0 * DACT_FP32_ERR[act] + _once(ref, dtype), act)
    if act == "relu":
        want = torch.where(u0.float() > 0, dh0.float(), torch.zeros(n)).to(dtype)
        got = du.cpu()
        assert torch.equal(got.float(), want.float()), "relu: du is dh where u > 0 and zero elsewhere, zero AT u = 0"
        assert float(got[0].float()) == 0.0 and float(got[1].float()) == 0.0 and float(got[3].float()) == 0.0
        assert float(got[2].float()) == float(dh0[2].float())


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_backward_applies_dact(dev, dtype):
    """ops.linear(x, w, b, act = GELU).backward: the stand-alone dact_mul (no following GEMM absorbs the derivative) between the saved
    pre-activation and the dgrad GEMM. dx = (dy * gelu'(u)) W against fp64, with the bound followed through the chain:
      u  = x W^T + b: K + 1 terms in fp32, stored in the compute type                      du_err = (K + 2) U32 sum|x w| + U |u|
      a  = gelu'(u):  |gelu''| <= 2 phi(0) < 0.8, the device formula within 8 x 1.44e-7    da = 0.8 du_err + 1.15e-6
      t  = dy * a, stored in the compute type                                              dt = |dy| da + (U + U32) |t|
      dx = t W: N terms in fp32, one rounding                                              sum |w| dt + (N + 1) U32 sum |t w| + U |dx|"""
    from valor_amd import lib, ops
    rows, K, N = 8, 64, 32
    g = torch.Generator().manual_seed(17)
    x0, w0, b0, dy0 = _randn(g, (rows, K), dtype), _randn(g, (N, K), dtype, 0.2), _randn(g, (N,), dtype), _randn(g, (rows, N), dtype)
    x = x0.to(dev).requires_grad_(True)
    y = ops.linear(x, w0.to(dev), b0.to(dev), act=lib.ACT_GELU_ERF)
    y.backward(dy0.to(dev))
    torch.cuda.synchronize()
    xr, wr, br, dyr = x0.double().requires_grad_(True), w0.double(), b0.double(), dy0.double()
    u = xr @ wr.t() + br
    (u * 0.5 * (1.0 + torch.erf(u * 0.7071067811865476))).backward(dyr)
    u = u.detach()
    du_err = (K + 2) * U32 * (xr.detach().abs() @ wr.abs().t() + br.abs()) + U(dtype) * u.abs()
    t = dyr * _dact(u, "gelu_erf")
    dt = dyr.abs() * (0.8 * du_err + 8.0 * DACT_FP32_ERR["gelu_erf"]) + (U(dtype) + U32) * t.abs()
    bound = dt @ wr.abs() + (N + 1) * U32 * (t.abs() @ wr.abs()) + U(dtype) * xr.grad.abs()
    _close(x.grad, xr.grad, bound, "dx")


# ------------------------------------------------------------------------------------------------ means, cast
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_mean_and_weighted_mean(dev, n):
    """valor_mean_f32: out = sum_i x[i] / n;  valor_weighted_mean_f32: out = sum_i w[i] x[i] / n (not / sum w) -- the kernels' header
    comments, in fp64. One 256-thread workgroup: n around one wave, around the workgroup, and 20 strides of it. Weights hold zeros and
    negatives."""
    _ptr, _stream, _ = _kp()
    g = torch.Generator().manual_seed(n)
    x0, w0 = 3.0 * torch.randn(n, generator=g) + 1.0, torch.randn(n, generator=g)
    w0[::3] = 0.0
    w0[n // 2] = -2.5
    x, w = x0.to(dev), w0.to(dev)
    m, wm = torch.full((), float("nan"), device=dev), torch.full((), float("nan"), device=dev)
    _call("valor_mean_f32", _stream(), _ptr(x), n, _ptr(m))
    _call("valor_weighted_mean_f32", _stream(), _ptr(x), _ptr(w), n, _ptr(wm))
    torch.cuda.synchronize()
    ref = x0.double().sum() / n
    wref = (w0.double() * x0.double()).sum() / n
    # n terms in fp32 (per-thread strides, a 64-lane tree, 4 wave partials: at most n + 9 additions), the products of the weighted sum
    # round once each, the division by n rounds once
    _close(m, ref, (n + 9) * U32 * x0.double().abs().sum() / n + U32 * ref.abs(), "mean")
    _close(wm, wref, (n + 10) * U32 * (w0.double() * x0.double()).abs().sum() / n + U32 * wref.abs(), "weighted mean")


def _cast_specials():
    """fp32 bit patterns around bf16's rounding: exact ties to an even and to an odd neighbour (both signs), just above / below a tie,
    the largest finite bf16, the tie above it (rounds to inf), values that round up into the next binade, +-0, +-inf, fp32 denormals
    (the smallest, one that ties, the largest) and the smallest normal"""
    pos = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x3F800000, 0x7F7F0000, 0x7F7F8000, 0x7F7F7FFF, 0x3FFFC000, 0x3FFF8000,
           0x407FFFFF, 0x00000000, 0x7F800000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x00010000]
    bits = pos + [b | 0x80000000 for b in pos]
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [40, GRID_ITEMS * 4 + 4])
def test_cast_from_f32(dev, dtype, n):
    """valor_cast_from_f32: the bf16 output is torch's round-to-nearest-even .to(torch.bfloat16) bit for bit on ties in both directions,
    the top of the range, binade carries, signed zeros, infinities and denormals; the fp32 output is a bit copy; n = 8 388 612: one
    four-element item past the grid cap, with the special values in the last items too."""
    _ptr, _stream, dt_of = _kp()
    sp = _cast_specials()
    g = torch.Generator().manual_seed(n)
    x0 = torch.randn(n, generator=g) * torch.exp(8.0 * torch.randn(n, generator=g))
    x0[:sp.numel()] = sp
    if n > 2 * sp.numel():
        x0[-sp.numel():] = sp
    out = torch.empty(n, dtype=dtype, device=dev)
    _call("valor_cast_from_f32", _stream(), dt_of(out), _ptr(x0.to(dev)), _ptr(out), n)
    _same_bits(out, x0.to(dtype), "cast")
