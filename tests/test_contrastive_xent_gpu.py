"""Kernel-level parity of contrastive.hip (fine-grained MGA similarity reduction + InfoNCE, model/pretrain.py:191-211,
model/modeling.py:418-433) and xent.hip (softmax cross-entropy on the vocabulary, model/pretrain.py:444) against fp64 torch math,
at the GLOBAL batch of the 8-GPU configuration (B = 512 pairs per side, 32 text tokens, Nv = 10 video + audio tokens) -- the
model-level tests only ever see B <= 4."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _ref_fine_loss(fa, fb, wa_raw, wb_raw, maskA, maskB, k):
    """compute_fine_matrix_slice + contrastive_loss in fp64 (masks multiply, max over v / over t, softmax token weights)"""
    wA = torch.softmax(wa_raw.masked_fill(maskA == 0, float("-inf")), dim=-1)
    wB = torch.softmax(wb_raw.masked_fill(maskB == 0, float("-inf")), dim=-1)
    logits = torch.einsum("atd,bvd->abtv", fa, fb)
    logits = logits * maskA[:, None, :, None] * maskB[None, :, None, :]
    a2b = logits.max(dim=-1)[0]
    b2a = logits.max(dim=-2)[0]
    score = (torch.einsum("abt,at->ab", a2b, wA) + torch.einsum("abv,bv->ab", b2a, wB)) / 2.0
    s = score * k
    l1 = (-F.log_softmax(s, dim=1)).diag()
    l2 = (-F.log_softmax(s, dim=0)).diag()
    return torch.mean(torch.cat((l1, l2), dim=0)), score


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("dtype,B,Nv", [(torch.float32, 512, 10), (torch.bfloat16, 512, 10), (torch.float32, 67, 8), (torch.float32, 5, 2)])
def test_fine_contrastive_at_global_batch(dev, dtype, B, Nv):
    from valor_amd import ops
    T, D = 32, 512
    g = torch.Generator().manual_seed(7)
    fa = F.normalize(torch.randn((B, T, D), generator=g), dim=-1).to(dtype).to(dev)
    fb = F.normalize(torch.randn((B, Nv, D), generator=g), dim=-1).to(dtype).to(dev)
    # correlated pairs so the diagonal is meaningful and the max / argmax are not degenerate
    fb = F.normalize(fb.float() + 0.5 * fa[:, :Nv].float(), dim=-1).to(dtype)
    wa_raw = torch.randn((B, T), generator=g).to(dev)
    wb_raw = torch.randn((B, Nv), generator=g).to(dev)
    lens = torch.randint(5, T + 1, (B,), generator=g)
    maskA = (torch.arange(T)[None, :] < lens[:, None]).float().to(dev)
    maskB = torch.ones((B, Nv), device=dev)
    k = torch.tensor(14.285, device=dev)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    a1, b1, wa1, wb1, k1 = leaf(fa), leaf(fb), leaf(wa_raw), leaf(wb_raw), leaf(k)
    loss = ops.fine_contrastive(a1, b1, wa1, wb1, maskA, maskB, k1)
    loss.backward()
    a2, b2, wa2, wb2, k2 = [leaf(t.double()) for t in (fa, fb, wa_raw, wb_raw, k)]
    ref, _ = _ref_fine_loss(a2, b2, wa2, wb2, maskA.double(), maskB.double(), k2)
    ref.backward()
    ltol, gtol = (2e-6, 2e-5) if dtype == torch.float32 else (2e-3, 2e-2)
    assert abs(float(loss) - float(ref)) <= ltol * abs(float(ref)), (float(loss), float(ref))
    for name, got, want in (("dfeatA", a1.grad, a2.grad), ("dfeatB", b1.grad, b2.grad), ("dwA", wa1.grad, wa2.grad),
                            ("dwB", wb1.grad, wb2.grad), ("dk", k1.grad, k2.grad)):
        assert _rel(got, want) < gtol, (name, _rel(got, want))
    # padded text positions carry no gradient to their weights
    assert float((wa1.grad * (1 - maskA)).abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_xent_against_fp64(dev, dtype):
    """valor_xent_fwd / _bwd on the padded-vocabulary layout the prediction head uses (V = 30522 in rows of 30528), labels incl. the
    first and last class, upstream gradient read from the device"""
    from valor_amd import lib
    from valor_amd.kernels import _ptr, _stream, dt_of
    n, V, Vpad = 1999, 30522, 30528
    g = torch.Generator().manual_seed(9)
    buf = torch.full((n, Vpad), float("nan"), dtype=dtype, device=dev)
    logits = (3.0 * torch.randn((n, V), generator=g)).to(dtype)
    buf[:, :V] = logits.to(dev)
    labels = torch.randint(0, V, (n,), generator=g)
    labels[0], labels[1] = 0, V - 1
    labels_d = labels.to(dev)
    loss_rows = torch.empty(n, dtype=torch.float32, device=dev)
    lse = torch.empty(n, dtype=torch.float32, device=dev)
    lib.call("valor_xent_fwd", _stream(), dt_of(buf), _ptr(buf), _ptr(labels_d), _ptr(loss_rows), _ptr(lse), n, V, Vpad)
    x = logits.double().requires_grad_(True)
    ref_rows = F.cross_entropy(x, labels, reduction="none")
    tol = 2e-6 if dtype == torch.float32 else 2e-5          # the statistics are fp32 in both modes; the INPUT is what is rounded
    assert _rel(loss_rows.cpu(), ref_rows) < tol
    assert _rel(lse.cpu(), torch.logsumexp(x, dim=-1)) < tol
    up = torch.tensor(0.37, device=dev)
    (0.37 * ref_rows.mean()).backward()
    lib.call("valor_xent_bwd", _stream(), dt_of(buf), _ptr(buf), _ptr(labels_d), _ptr(lse), _ptr(up), 1.0 / n, n, V, Vpad)
    assert _rel(buf[:, :V].cpu(), x.grad) < (2e-6 if dtype == torch.float32 else 4e-3)
    assert float(buf[:, V:].float().abs().max()) == 0.0     # the ld padding is zero-filled (it is a GEMM operand next)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_label_smoothing_cross_entropy(dev, dtype):
    """valor_xent_smooth_fwd / _bwd (LabelSmoothing, model/pretrain.py:46-61): row loss = KL(smoothed target || softmax) and its gradient
    against fp64, on the padded-vocabulary layout; smoothing 0 reproduces valor_xent_fwd / _bwd bit for bit."""
    from valor_amd import lib
    from valor_amd.kernels import _ptr, _stream, dt_of
    n, V, Vpad, eps = 37, 30522, 30528, 0.1
    g = torch.Generator().manual_seed(2)
    logits = (3.0 * torch.randn((n, Vpad), generator=g)).to(dtype)
    labels = torch.randint(0, V, (n,), generator=g)
    buf = logits.to(dev).clone()
    lab_d = labels.to(dev)
    loss_rows = torch.empty(n, device=dev); lse = torch.empty(n, device=dev)
    lib.call("valor_xent_smooth_fwd", _stream(), dt_of(buf), _ptr(buf), _ptr(lab_d), _ptr(loss_rows), _ptr(lse), n, V, Vpad, eps)
    z = logits[:, :V].double().requires_grad_(True)
    logp = torch.log_softmax(z, -1)
    tgt = torch.full_like(logp, eps / (V - 1)); tgt.scatter_(1, labels.unsqueeze(1), 1.0 - eps)
    ref_rows = (tgt * (tgt.log() - logp)).sum(1)
    assert torch.allclose(loss_rows.cpu().double(), ref_rows.detach(), rtol=2e-4, atol=2e-4), (loss_rows[:4], ref_rows[:4])
    ref_rows.mean().backward()
    up = torch.full((), 1.0, device=dev)
    lib.call("valor_xent_smooth_bwd", _stream(), dt_of(buf), _ptr(buf), _ptr(lab_d), _ptr(lse), _ptr(up), 1.0 / n, n, V, Vpad, eps)
    got = buf[:, :V].cpu().double()
    tol = 2e-6 if dtype == torch.float32 else 2e-2
    assert float((got - z.grad).norm() / z.grad.norm()) < tol
    assert float(buf[:, V:].float().abs().max()) == 0.0
    # smoothing 0 == the plain entry points, bit for bit
    a, b = logits.to(dev).clone(), logits.to(dev).clone()
    la, lb = torch.empty(n, device=dev), torch.empty(n, device=dev)
    sa, sb = torch.empty(n, device=dev), torch.empty(n, device=dev)
    lib.call("valor_xent_smooth_fwd", _stream(), dt_of(a), _ptr(a), _ptr(lab_d), _ptr(la), _ptr(sa), n, V, Vpad, 0.0)
    lib.call("valor_xent_fwd", _stream(), dt_of(b), _ptr(b), _ptr(lab_d), _ptr(lb), _ptr(sb), n, V, Vpad)
    assert torch.equal(la, lb) and torch.equal(sa, sb)


# ------------------------------------------------------------------------------------------------ cross-entropy edges
# Everything below runs on the padded layout (V columns in rows of ld, the pad NaN before the forward) and compares ELEMENTWISE,
# |got - ref| <= 2 * bound, with the bound taken from the arithmetic: U32 = 2^-24 per fp32 rounding, n * U32 * sum |term| for a sum of n
# terms accumulated in fp32, one half-ulp of the output type for the stored gradient. expf / logf are the exception: their error is
# measured -- the kernel's formula (mx = max z; S = sum exp(z - mx); lse = mx + log S) evaluated by torch in fp32 on the CPU against fp64
# on the inputs of these tests (all shapes, the range rows, fp32 and bf16-rounded logits pooled; arguments below -80, whose exp is under
# 1e-34 of the row's sum, left out): exp differs by at most 5.99e-8 relative, log S by at most 7.8e-8 and the log of the smoothing
# constants (log(eps / (V - 1)), log(1 - eps)) by at most 2.24e-7 absolute. The kernel may use another few-ulp implementation: 8 x each.
U32 = 2.0 ** -24
XENT_EXP_REL = 8 * 6.0e-8            # 4.8e-7
XENT_LOG_ABS = 8 * 2.3e-7            # 1.84e-6
XENT_SHAPES = [(1, 32), (2, 32), (255, 256), (256, 256), (257, 288), (1000, 1024)]
XENT_W = [1.0, 0.0, -0.75, 40.0, 0.3, -2.0, 1.5]         # per-row weights of the weighted backward: a zero, negatives, a large one


def _close(got, ref, bound, what):
    got, ref, bound = got.detach().double().cpu(), ref.detach().double().cpu(), bound.detach().double().cpu().expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ok = (got - ref).abs() <= 2.0 * bound
    if not bool(ok.all()):
        i = int((~ok).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements off, first at flat index {i}: got {got.flatten()[i]!r} "
                             f"want {ref.flatten()[i]!r} allowed {2.0 * bound.flatten()[i]!r}")


def _xent_ref_rows(z, labels, eps):
    """row losses in fp64 (differentiable in z): -logp[label], or KL(smoothed target || softmax); 0 for a label outside [0, V)"""
    V = z.shape[1]
    valid = (labels >= 0) & (labels < V)
    lab = labels.clamp(0, V - 1).unsqueeze(1)
    logp = torch.log_softmax(z, -1)
    rows = -logp.gather(1, lab)[:, 0]
    if eps > 0:
        tgt = torch.full_like(logp, eps / (V - 1)).scatter(1, lab, 1.0 - eps)
        rows = (tgt * (tgt.log() - logp)).sum(1)
    return torch.where(valid, rows, torch.zeros_like(rows)), valid


def _check_xent(dev, z0, labels, ld, backward=True):
    """forward (plain; smoothed with eps = 0.1 if V > 1) and the plain / smoothed / weighted backward, each with the upstream gradient as
    a device scalar and as null, of logits z0 [n, V] (already in the type under test) against fp64; returns the gradients it checked"""
    from valor_amd import lib
    from valor_amd.kernels import _ptr, _stream, dt_of
    n, V = z0.shape
    dtype = z0.dtype
    u_out = 2.0 ** -9 if dtype == torch.bfloat16 else U32
    lab_d = labels.to(dev)

    def padded():
        buf = torch.full((n, ld), float("nan"), dtype=dtype, device=dev)
        buf[:, :V] = z0.to(dev)
        return buf

    zd = z0.double()
    lse_ref = torch.logsumexp(zd, -1)
    # lse = mx + log S: S sums V exponentials in fp32 (relative V U32) of arguments z - mx that are exact where they matter (Sterbenz) and
    # each carry expf's error; log S: d S / S + logf's error; the last addition rounds once
    b_lse = (V + 1) * U32 + XENT_EXP_REL + XENT_LOG_ABS + U32 * lse_ref.abs()
    grads = {}
    for eps in (0.0, 0.1) if V > 1 else (0.0,):
        buf = padded()
        loss = torch.full((n,), float("nan"), device=dev)
        lse = torch.full((n,), float("nan"), device=dev)
        if eps == 0.0:
            lib.call("valor_xent_fwd", _stream(), dt_of(buf), _ptr(buf), _ptr(lab_d), _ptr(loss), _ptr(lse), n, V, ld)
        else:
            lib.call("valor_xent_smooth_fwd", _stream(), dt_of(buf), _ptr(buf), _ptr(lab_d), _ptr(loss), _ptr(lse), n, V, ld, eps)
        ref_rows, valid = _xent_ref_rows(zd, labels, eps)
        _close(lse, lse_ref, b_lse, f"lse (eps {eps})")            # written for every row, ignored ones included
        nll = torch.where(valid, lse_ref - zd.gather(1, labels.clamp(0, V - 1).unsqueeze(1))[:, 0], torch.zeros(n, dtype=torch.float64))
        b_nll = b_lse + U32 * nll.abs()                              # lse - z[label]: one more rounding
        if eps == 0.0:
            b_loss = b_nll
        else:
            # (1-eps) log(1-eps) + eps log u + (1-eps) nll - u (sum_j logp_j + nll), u = eps / (V-1), sum_j logp_j = sum z - V lse:
            # sum z accumulates V terms; V lse carries V b_lse; two logf of constants; every product / sum of the expression rounds once
            u = eps / (V - 1)
            sz = zd.sum(-1)
            slp = sz - V * lse_ref
            b_slp = V * U32 * zd.abs().sum(-1) + V * b_lse + 2 * U32 * (sz.abs() + V * lse_ref.abs())
            terms = (1 - eps) * abs(math.log(1 - eps)) + eps * abs(math.log(u)) + (1 - eps) * nll.abs() + u * (slp + nll).abs()
            b_loss = u * (b_slp + b_nll) + (1 - eps) * b_nll + XENT_LOG_ABS + 4 * U32 * terms
        b_loss = torch.where(valid, b_loss, torch.zeros_like(b_loss))            # an ignored row's loss is exactly 0
        _close(loss, ref_rows, b_loss, f"loss rows (eps {eps})")
        assert bool(torch.isnan(buf[:, V:].float()).all()) and torch.equal(buf[:, :V].cpu(), z0), "the forward does not write the logits"
        if not backward:
            continue
        w0 = torch.tensor((XENT_W * (n // len(XENT_W) + 1))[:n])
        w_d = w0.to(dev)
        for entry in ("plain", "weighted") if eps == 0.0 else ("smooth",):
            for up in (0.37, None):
                gmul = 1.0 / n                 # the caller's mean over ITS row count: the kernel does not renormalise by the valid rows
                g_rows = torch.full((n,), (up if up is not None else 1.0) * gmul, dtype=torch.float64)
                if entry == "weighted":
                    g_rows = g_rows * w0.double()
                zr = zd.clone().requires_grad_(True)
                (_xent_ref_rows(zr, labels, eps)[0] * g_rows).sum().backward()
                buf = padded()
                up_d = torch.tensor(up, device=dev) if up is not None else None
                if entry == "plain":
                    lib.call("valor_xent_bwd", _stream(), dt_of(buf), _ptr(buf), _ptr(lab_d), _ptr(lse), _ptr(up_d), gmul, n, V, ld)
                elif entry == "smooth":
                    lib.call("valor_xent_smooth_bwd", _stream(), dt_of(buf), _ptr(buf), _ptr(lab_d), _ptr(lse), _ptr(up_d), gmul, n, V, ld, eps)
                else:
                    lib.call("valor_xent_weighted_bwd", _stream(), dt_of(buf), _ptr(buf), _ptr(lab_d), _ptr(lse), _ptr(w_d), _ptr(up_d),
                             gmul, n, V, ld)
                # d = (exp(z - lse) - t) g with the FORWARD's lse (within 2 b_lse): the argument errs by that and its own rounding, expf
                # by its relative error -> p (2 b_lse + U32 |z - lse| + exp); results under the normal range (2^-126) may be flushed; the
                # subtraction rounds once, t = eps / (V - 1) and g = up * gmul * w carry two roundings each; one product, one store
                p = torch.softmax(zd, -1)
                tgt = torch.zeros_like(p).scatter(1, labels.clamp(0, V - 1).unsqueeze(1), 1.0)
                if eps > 0:
                    tgt = torch.full_like(p, eps / (V - 1)).scatter(1, labels.clamp(0, V - 1).unsqueeze(1), 1.0 - eps)
                dp = p * (2 * b_lse[:, None] + U32 * (zd - lse_ref[:, None]).abs() + XENT_EXP_REL) + 2.0 ** -126
                bound = g_rows.abs()[:, None] * (dp + U32 * (p - tgt).abs() + 2 * U32 * tgt) + zr.grad.abs() * (3 * U32 + u_out) + 2.0 ** -126
                bound = torch.where(valid[:, None], bound, torch.zeros_like(bound))     # an ignored row: exact zeros
                what = f"{entry} backward, upstream {up}"
                _close(buf[:, :V], zr.grad, bound, what)
                assert not bool((buf[:, V:] != 0).any()), what + ": the ld padding is zero-filled"
                if not bool(valid.all()):
                    assert float(buf[~valid.to(dev)].float().abs().max()) == 0.0, what + ": an ignored row is zero, pad included"
                grads[(entry, up)] = buf.cpu()
    return grads


def _xent_logits(V, dtype):
    g = torch.Generator().manual_seed(V * 31)
    z0 = (3.0 * torch.randn((7, V), generator=g)).to(dtype)
    labels = torch.randint(0, V, (7,), generator=g)
    labels[0], labels[1] = 0, V - 1
    return z0, labels


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,ld", XENT_SHAPES)
def test_xent_small_and_unaligned_vocabulary(dev, dtype, V, ld):
    """7 rows of V = 1 / 2 (fewer columns than the 256 threads that walk a row), 255 / 256 / 257 (one short of, exactly, one into the
    second pass) and 1000 classes in rows of ld: loss, lse, the gradient of the plain, smoothed (eps 0.1; not at V = 1, where the entry
    point refuses it) and weighted (weights 0, negative, 40) backward with the upstream gradient on the device and null, the zero pad.
    Transcendental allowance (measured, see above): exp 8 x 5.99e-8 = 4.8e-7 relative, log 8 x 2.3e-7 = 1.84e-6 absolute."""
    z0, labels = _xent_logits(V, dtype)
    _check_xent(dev, z0, labels, ld)


def test_xent_wide_range_rows(dev):
    """fp32 rows that only the max-subtraction keeps finite: logits uniform over +-1e4, a row of identical values (lse = c + log V),
    one +1e4 and one -1e4 among N(0, 1), whole rows shifted to -1e4 and +1e4, an even ramp from -1e4 to 1e4: lse and loss against fp64
    (the fp32 rounding of an lse near 1e4 is 6e-4: the U32 |lse| term of the bound)."""
    V, ld = 257, 288
    g = torch.Generator().manual_seed(99)
    z = torch.empty(6, V)
    z[0] = (torch.rand(V, generator=g) * 2 - 1) * 1e4
    z[1] = 123.456
    z[2] = torch.randn(V, generator=g); z[2, 7] = 1e4; z[2, 9] = -1e4
    z[3] = -1e4 + torch.randn(V, generator=g)
    z[4] = 1e4 + 3 * torch.randn(V, generator=g)
    z[5] = torch.linspace(-1e4, 1e4, V)
    labels = torch.tensor([int(z[0].argmin()), 5, 9, 0, V - 1, 0])
    _check_xent(dev, z, labels, ld, backward=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_xent_ignored_rows(dev, dtype):
    """A label outside [0, V) (-1 and V) marks an ignored row, in the forward AND the backward: loss 0, lse still written, a gradient row
    of exact zeros (pad included) from all three backward entry points whatever the row weight; the other rows' gradients are bit for
    bit what they are when every label is valid -- still scaled by the caller's gmul = 1 / n, not renormalised by the valid rows."""
    V, ld = 257, 288
    z0, labels = _xent_logits(V, dtype)
    ign = labels.clone()
    ign[2], ign[3], ign[5] = -1, V, -1                      # row 3 carries the weight 40, rows 2 and 5 negative ones
    got = _check_xent(dev, z0, ign, ld)
    full = _check_xent(dev, z0, labels, ld)
    keep = torch.tensor([0, 1, 4, 6])
    assert set(got) == {(e, u) for e in ("plain", "weighted", "smooth") for u in (0.37, None)}
    for key, gbuf in got.items():
        assert torch.equal(gbuf[keep], full[key][keep]), key
        assert float(gbuf[[2, 3, 5]].float().abs().max()) == 0.0 and float(full[key][[2, 3, 5]].float().abs().max()) > 0.0, key
