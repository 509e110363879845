"""Where a parameter's gradient goes, op by op: ops.linear, ops.mlp and the three tied-decoder loss entry points (decoder_xent,
decoder_xent_segments, decoder_xent_weighted_segments) on every gradient route -- returned to autograd ("ret"), accumulated by the
producing kernel into an arena slot that already holds something ("sink": ops.GradSink, what the model does; "rec": the same while a
backward is being captured, ops.GradSink.recorder), weight and bias frozen ("frozen": no gradient launch at all), and, for linear and
mlp, two nodes whose input gradients meet in one ops.GradSlot ("slot").

Checked: values against the same expression in fp64 torch autograd (relative norms, the tolerances of test_embed_ops_gpu.py), which
parameter names are reported and to whom, which launches run (the recorded lib.call stream), the memory around a gradient slot, and the
exact relations between the loss entry points. Shapes are the smallest on which each branch is taken: 96 x 64 x 80 products stay on the
128 x 128 kernels, whose bias gradient is a column sum; 4096 x 256 x 256 is the smallest wgrad valor_gemm_kernel_for hands to the 8-phase
kernel (M, N >= 256, K = rows >= 4096), which produces the bias gradient as fused row sums.

run_linear / run_mlp / run_loss and the case tables are also what tools/ops_trace.py replays."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PAD = 64                                   # guard elements on either side of a gradient slot
OUT_TOL = {torch.float32: 1e-6, torch.bfloat16: 4e-3}
GRAD_TOL = {torch.float32: 1e-5, torch.bfloat16: 1.2e-2}
FUSING = (4096, 256, 256)                  # (rows, in, out): smallest bf16 wgrad with fused row sums (asserted where it is used)
PLAIN = (96, 64, 80)

# (dtype, w_is_kn, (rows, in, out), act) -- act by name: lib.ACT_*
LINEAR_CASES = [(dt, kn, PLAIN, act) for dt in (torch.float32, torch.bfloat16) for kn in (False, True) for act in ("ACT_GELU_ERF", "ACT_NONE")] \
    + [(torch.bfloat16, False, FUSING, "ACT_NONE")]
# (dtype, (rows, in, inter, out))
MLP_CASES = [(dt, shp) for dt in (torch.float32, torch.bfloat16) for shp in ((96, 64, 80, 48), (4096, 256, 256, 256))]
# (dtype, kind, smoothing); n = 37 rows, hidden 64, V = 50 (rows of Vpad = 64 logits), segments [20, 17]
LOSS_N, LOSS_H, LOSS_V, LOSS_SEGS = 37, 64, 50, (20, 17)
LOSS_CASES = [(dt, kind, sm) for dt in (torch.float32, torch.bfloat16) for kind in ("plain", "segments") for sm in (0.0, 0.1)] \
    + [(dt, "weighted", 0.0) for dt in (torch.float32, torch.bfloat16)]
ROUTES = ("ret", "sink", "rec", "frozen")


def _id(v):
    return str(v).replace("torch.", "").replace(" ", "")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _randn(shape, g, dtype, dev, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).to(dtype).to(dev)


class Leaf:
    """a parameter-like leaf. On the sink routes it looks like an arena parameter: `_arena_name`, and a gradient slot in the middle of a
    larger buffer that already holds `g0`; `guards_untouched()` says whether the memory around the slot still holds what it held."""

    def __init__(self, t, route, name, g):
        self.p = t.clone().requires_grad_(route != "frozen")
        self.name, self.g0, self.flat = name, None, None
        if route != "ret":
            self.p._arena_name = name
        if route in ("sink", "rec"):
            self.flat = _randn((t.numel() + 2 * PAD,), g, t.dtype, t.device, 0.5)
            self.before = self.flat.clone()
            self.p.grad = self.flat[PAD:PAD + t.numel()].view(t.shape)
            self.g0 = self.p.grad.clone()

    def guards_untouched(self):
        return torch.equal(self.flat[:PAD], self.before[:PAD]) and torch.equal(self.flat[-PAD:], self.before[-PAD:])


@contextlib.contextmanager
def recording(route="sink"):
    """-> (calls, seen, recorded): every lib.call as (name, args) while it is forwarded, the names GradSink.listener is told, and the
    names that land in GradSink.recorder (route "rec": a list for the duration, as during the capture of a backward pass)"""
    from valor_amd import lib, ops
    calls, seen, recorded = [], [], []
    real, old_l, old_r = lib.call, ops.GradSink.listener, ops.GradSink.recorder

    def call(name, *args):
        calls.append((name, args))
        return real(name, *args)

    lib.call, ops.GradSink.listener = call, seen.append
    if route == "rec":
        ops.GradSink.recorder = recorded
    try:
        yield calls, seen, recorded
    finally:
        lib.call, ops.GradSink.listener, ops.GradSink.recorder = real, old_l, old_r


def _finish():
    from valor_amd import kernels as K
    K.ReduceQueue.flush_all()
    torch.cuda.synchronize()


def _is_gemm(name):
    return name in ("valor_gemm", "valor_gemm_deferred", "valor_gemm_tuned")


def _gemm_arg(call, i):
    """argument i of a valor_gemm / valor_gemm_deferred call (2: transA, 3: transB, 19: accumulate); valor_gemm_tuned has one more in front"""
    name, args = call
    return args[i + 1] if name == "valor_gemm_tuned" else args[i]


def wgrad_and_colsum_calls(calls):
    return [c[0] for c in calls if c[0] == "valor_colsum" or (_is_gemm(c[0]) and _gemm_arg(c, 2) == 1 and _gemm_arg(c, 3) == 1)]


def _act64(name, u):
    return F.gelu(u) if name == "ACT_GELU_ERF" else u


# ------------------------------------------------------------------------------------------------ linear / mlp
def run_linear(dev, case, route):
    from valor_amd import lib, ops
    dtype, kn, (rows, nin, nout), act = case
    g = torch.Generator().manual_seed(rows + nin + nout)
    x0 = _randn((rows, nin), g, dtype, dev)
    w0 = _randn((nin, nout) if kn else (nout, nin), g, dtype, dev, nin ** -0.5)
    b0 = _randn((nout,), g, dtype, dev)
    dy = _randn((rows, nout), g, dtype, dev)
    x = x0.clone().requires_grad_(True)
    w, b = Leaf(w0, route, "w", g), Leaf(b0, route, "b", g)
    with recording(route) as (calls, seen, recorded):
        y = ops.linear(x, w.p, b.p, act=getattr(lib, act), w_is_kn=kn)
        y.backward(dy)
        _finish()

    xr, wr, br = (t.double().requires_grad_(True) for t in (x0, w0, b0))
    ref = _act64(act, xr @ (wr if kn else wr.t()) + br)
    ref.backward(dy.double())
    return dict(out=y, ref=ref, x=(x, xr), leaves=((w, wr), (b, br)), calls=calls, seen=seen, recorded=recorded)


def run_mlp(dev, case, route):
    from valor_amd import lib, ops
    dtype, (rows, nin, inter, nout) = case
    g = torch.Generator().manual_seed(rows + nin + inter + nout)
    x0 = _randn((rows, nin), g, dtype, dev)
    w10, b10 = _randn((inter, nin), g, dtype, dev, nin ** -0.5), _randn((inter,), g, dtype, dev)
    w20, b20 = _randn((nout, inter), g, dtype, dev, inter ** -0.5), _randn((nout,), g, dtype, dev)
    dy = _randn((rows, nout), g, dtype, dev)
    x = x0.clone().requires_grad_(True)
    ls = [Leaf(t, route, n, g) for t, n in ((w10, "w1"), (b10, "b1"), (w20, "w2"), (b20, "b2"))]
    with recording(route) as (calls, seen, recorded):
        y = ops.mlp(x, *(l.p for l in ls), lib.ACT_GELU_ERF)
        y.backward(dy)
        _finish()

    xr, w1r, b1r, w2r, b2r = (t.double().requires_grad_(True) for t in (x0, w10, b10, w20, b20))
    ref = F.gelu(xr @ w1r.t() + b1r) @ w2r.t() + b2r
    ref.backward(dy.double())
    return dict(out=y, ref=ref, x=(x, xr), leaves=tuple(zip(ls, (w1r, b1r, w2r, b2r))), calls=calls, seen=seen, recorded=recorded)


def run_slot(dev, op, case):
    """two nodes of `op` ("linear" / "mlp") on ONE activation, sharing a GradSlot; parameter gradients are returned to autograd"""
    from valor_amd import lib, ops
    if op == "linear":
        dtype, kn, (rows, nin, nout), act = case
        shapes = [((nin, nout) if kn else (nout, nin), nin ** -0.5), ((nout,), 1.0)]
    else:
        dtype, (rows, nin, inter, nout) = case
        shapes = [((inter, nin), nin ** -0.5), ((inter,), 1.0), ((nout, inter), inter ** -0.5), ((nout,), 1.0)]
    g = torch.Generator().manual_seed(7 + rows)
    x0 = _randn((rows, nin), g, dtype, dev)
    prm = [[_randn(s, g, dtype, dev, sc) for s, sc in shapes] for _ in range(2)]
    dys = [_randn((rows, nout), g, dtype, dev) for _ in range(2)]
    x_leaf = x0.clone().requires_grad_(True)
    x = x_leaf * 1.0                       # a non-leaf, as in the model: its producer gets ONE gradient, after both consumers ran
    slot, returned, ys = ops.GradSlot(), [], []
    leaves = [[t.clone().requires_grad_(True) for t in ps] for ps in prm]
    with recording() as (calls, seen, _):
        for ps in leaves:
            y = ops.linear(x, *ps, act=getattr(lib, act), w_is_kn=kn, grad_slot=slot) if op == "linear" \
                else ops.mlp(x, *ps, lib.ACT_GELU_ERF, grad_slot=slot)
            y.grad_fn.register_hook(lambda gin, gout: returned.append(gin[0] is not None))
            ys.append(y)
        torch.autograd.backward(ys, dys)
        _finish()

    xr = x0.double().requires_grad_(True)
    for ps, dy in zip(prm, dys):
        ps = [t.double() for t in ps]
        if op == "linear":
            ref = _act64(act, xr @ (ps[0] if kn else ps[0].t()) + ps[1])
        else:
            ref = F.gelu(xr @ ps[0].t() + ps[1]) @ ps[2].t() + ps[3]
        ref.backward(dy.double())
    return dict(x=(x_leaf, xr), outs=ys, leaves=leaves, calls=calls, seen=seen, returned=returned)


def _check(r, dtype, route, names):
    """values, reports and launches of one run_linear / run_mlp / run_loss result"""
    out_tol, tol = OUT_TOL[dtype], GRAD_TOL[dtype]
    outs = r["out"] if isinstance(r["out"], (tuple, list)) else (r["out"],)
    refs = r["ref"] if isinstance(r["ref"], (tuple, list)) else (r["ref"],)
    for i, (o, f) in enumerate(zip(outs, refs)):
        e = _rel(o, f)
        print(f"out[{i}] rel {e:.3e} (tol {out_tol:.1e})")
        assert e < out_tol, (i, e)
    x, xr = r["x"]
    e = _rel(x.grad, xr.grad)
    print(f"dx rel {e:.3e} (tol {tol:.1e})")
    assert e < tol, e
    for leaf, ref in r["leaves"]:
        if route == "frozen":
            assert leaf.p.grad is None, leaf.name
            continue
        want = ref.grad + (leaf.g0.double() if leaf.g0 is not None else 0.0)
        e = _rel(leaf.p.grad, want)
        print(f"d{leaf.name} rel {e:.3e} (tol {tol:.1e})")
        assert e < tol, (leaf.name, e)
        if leaf.flat is not None:
            assert leaf.guards_untouched(), leaf.name          # nothing was written around the gradient slot
    sunk = sorted(names)
    assert sorted(r["seen"]) == (sunk if route == "sink" else []), r["seen"]            # each sunk parameter once, nobody else
    assert sorted(r["recorded"]) == (sunk if route == "rec" else []), r["recorded"]      # during a capture: recorded, not reported
    if route == "frozen":
        assert wgrad_and_colsum_calls(r["calls"]) == []


def _assert_fuses(dtype, rows, m, n):
    from valor_amd import kernels as K
    dy, x = torch.empty((rows, m), dtype=dtype, device="cuda"), torch.empty((rows, n), dtype=dtype, device="cuda")
    assert K.gemm_fuses_rowsum(dy, x, True, True), (rows, m, n)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", LINEAR_CASES, ids=_id)
def test_linear(dev, case, route):
    dtype, kn, (rows, nin, nout), act = case
    if (rows, nin, nout) == FUSING:
        _assert_fuses(dtype, rows, nout, nin)
    r = run_linear(dev, case, route)
    _check(r, dtype, route, ("w", "b"))
    n_colsum = sum(c[0] == "valor_colsum" for c in r["calls"])
    if route != "frozen":                  # the bias gradient rides the wgrad GEMM exactly where the kernel offers it and a slot takes it
        assert n_colsum == (0 if (rows, nin, nout) == FUSING and route != "ret" else 1)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", MLP_CASES, ids=_id)
def test_mlp(dev, case, route):
    dtype, (rows, nin, inter, nout) = case
    fusing = rows == FUSING[0] and dtype == torch.bfloat16
    if fusing:
        _assert_fuses(dtype, rows, nout, inter)
        _assert_fuses(dtype, rows, inter, nin)
    r = run_mlp(dev, case, route)
    _check(r, dtype, route, ("w1", "b1", "w2", "b2"))
    if route != "frozen":
        assert sum(c[0] == "valor_colsum" for c in r["calls"]) == (0 if fusing and route != "ret" else 2)


@pytest.mark.parametrize("op,case", [("linear", c) for c in LINEAR_CASES] + [("mlp", c) for c in MLP_CASES], ids=_id)
def test_two_nodes_share_a_grad_slot(dev, op, case):
    dtype = case[0]
    r = run_slot(dev, op, case)
    x, xr = r["x"]
    e = _rel(x.grad, xr.grad)
    print(f"dx rel {e:.3e} (tol {GRAD_TOL[dtype]:.1e})")
    assert e < GRAD_TOL[dtype], e
    assert sorted(r["returned"]) == [False, True]              # one backward produced the buffer, the other added into it
    assert sum(_is_gemm(c[0]) and _gemm_arg(c, 19) == 1 for c in r["calls"]) == 1
    assert r["seen"] == []


# ------------------------------------------------------------------------------------------------ tied-decoder loss
def _loss_inputs(dev, dtype):
    n, H, V = LOSS_N, LOSS_H, LOSS_V
    g = torch.Generator().manual_seed(21)
    h0 = _randn((n, H), g, dtype, dev)
    w0 = _randn((V, H), g, dtype, dev, H ** -0.5)
    b0 = _randn((V,), g, dtype, dev, 0.1)
    labels = torch.randint(0, V, (n,), generator=g)
    labels[0], labels[1] = 0, V - 1
    w_rows = torch.randn(n, generator=g)
    w_rows[3], w_rows[5] = 0.0, -1.5                           # a row without weight, a negative reward
    return g, h0, w0, b0, labels.to(dev), w_rows.to(dev)


def _loss_ref(h0, w0, b0, labels, segs, smoothing, w_rows):
    hr, wr, br = (t.double().requires_grad_(True) for t in (h0, w0, b0))
    logits = hr @ wr.t() + br
    logp = F.log_softmax(logits, dim=-1)
    V = logp.shape[1]
    tgt = torch.full_like(logp, smoothing / (V - 1)).scatter_(1, labels.unsqueeze(1), 1.0 - smoothing)
    rows = (torch.xlogy(tgt, tgt) - tgt * logp).sum(-1)          # KL(smoothed target || softmax) (LabelSmoothing, pretrain.py:46-61); smoothing 0: CE
    if w_rows is not None:
        rows = rows * w_rows.double()
    losses, r0 = [], 0
    for nr in segs:
        losses.append(rows[r0:r0 + nr].sum() / nr); r0 += nr
    return (hr, wr, br), losses, logits.detach(), -logp.detach().gather(1, labels.unsqueeze(1)).squeeze(1)


SEG_COEF = (1.0, 0.7)                      # d(total) / d(segment loss): the segments get different upstream gradients


def run_loss(dev, case, route, want_logits=False):
    from valor_amd import ops
    dtype, kind, smoothing = case
    g, h0, w0, b0, labels, w_rows = _loss_inputs(dev, dtype)
    segs = (LOSS_N,) if kind == "plain" else LOSS_SEGS
    h = h0.clone().requires_grad_(True)
    w, b = Leaf(w0, route, "w", g), Leaf(b0, route, "b", g)
    extra = {}
    with recording(route) as (calls, seen, recorded):
        if kind == "plain":
            res = ops.decoder_xent(h, w.p, b.p, labels, want_logits=want_logits, smoothing=smoothing)
            losses = (res[0],) if want_logits else (res,)
            if want_logits:
                extra["logits"] = res[1].clone()               # (backward overwrites the buffer in place)
        elif kind == "segments":
            losses = ops.decoder_xent_segments(h, w.p, b.p, labels, list(segs), smoothing=smoothing)
        else:
            rows_out = []
            losses = ops.decoder_xent_weighted_segments(h, w.p, b.p, labels, list(segs), w_rows, loss_rows_out=rows_out)
            extra["rows"] = rows_out[0]
        assert isinstance(losses, tuple) and len(losses) == len(segs)
        sum(c * l for c, l in zip(SEG_COEF, losses)).backward()
        _finish()

    (hr, wr, br), ref, ref_logits, ref_rows = _loss_ref(h0, w0, b0, labels, segs, smoothing, w_rows if kind == "weighted" else None)
    sum(c * l for c, l in zip(SEG_COEF, ref)).backward()
    return dict(out=tuple(l.detach() for l in losses), ref=tuple(l.detach() for l in ref), x=(h, hr), leaves=((w, wr), (b, br)),
                calls=calls, seen=seen, recorded=recorded, ref_logits=ref_logits, ref_rows=ref_rows, **extra)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", LOSS_CASES, ids=_id)
def test_decoder_loss(dev, case, route):
    dtype, kind, smoothing = case
    r = run_loss(dev, case, route)
    _check(r, dtype, route, ("w", "b"))
    if kind == "weighted":                 # the per-row CE: -logP of each label, no gradient
        assert not r["rows"].requires_grad and r["rows"].shape == (LOSS_N,)
        assert _rel(r["rows"], r["ref_rows"]) < OUT_TOL[dtype]
    names = {c[0] for c in r["calls"]}
    if kind == "weighted":                 # the weighted node runs its own kernels, not the smoothing ones with smoothing 0
        assert {"valor_xent_fwd", "valor_weighted_mean_f32", "valor_xent_weighted_bwd"} <= names and "valor_xent_smooth_bwd" not in names
    else:
        assert {"valor_xent_smooth_fwd", "valor_mean_f32", "valor_xent_smooth_bwd"} <= names
    assert not any(c[0] in ("valor_gemm", "valor_gemm_deferred") and c[1][23] for c in r["calls"])      # these products never fuse row sums


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_id)
def test_plain_loss_is_the_one_segment_loss(dev, dtype, smoothing, route):
    """decoder_xent(h, ...) and decoder_xent_segments(h, ..., [n])[0]: the same bits in the loss, dh and the weight and bias gradients;
    with want_logits the logits are decoder_logits'."""
    from valor_amd import ops
    a = run_loss(dev, (dtype, "plain", smoothing), route, want_logits=True)
    g, h0, w0, b0, labels, _ = _loss_inputs(dev, dtype)
    h = h0.clone().requires_grad_(True)
    w, b = Leaf(w0, route, "w", g), Leaf(b0, route, "b", g)         # the same generator state: the same g0 as in `a`
    with recording(route) as (calls, seen, recorded):
        (loss,) = ops.decoder_xent_segments(h, w.p, b.p, labels, [LOSS_N], smoothing=smoothing)
        (SEG_COEF[0] * loss).backward()
        _finish()
    assert torch.equal(loss.detach(), a["out"][0])
    assert torch.equal(h.grad, a["x"][0].grad)
    for mine, (theirs, _) in zip((w, b), a["leaves"]):
        if route == "frozen":
            assert mine.p.grad is None and theirs.p.grad is None
        else:
            assert torch.equal(mine.p.grad, theirs.p.grad), mine.name
    assert (sorted(seen), sorted(recorded)) == (sorted(a["seen"]), sorted(a["recorded"]))
    strip = lambda cs: [(n, tuple(v for v in args if isinstance(v, float) or (isinstance(v, int) and abs(v) < 1 << 20))) for n, args in cs]
    assert strip(calls) == strip(a["calls"])                        # call for call (names, sizes, flags; addresses aside)
    assert torch.equal(a["logits"], ops.decoder_logits(h0, w0, b0))
    assert _rel(a["logits"], a["ref_logits"]) < OUT_TOL[dtype]
