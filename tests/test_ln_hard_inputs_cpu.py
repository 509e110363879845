"""tests/ln_hard_inputs.py held to its purpose, without a GPU:
 (1) the row classes have the properties they are named for, on the fp64 reference;
 (2) an fp32 restatement of the kernels' summation order (per-lane sequential adds, a butterfly over the lane group, the column sums through
     per-workgroup partials and colsum_finalize's 4 x 16 + tree order) passes the judge on every class, both eps, both dtypes, with its largest
     observed / allowed ratio below 0.6 in every output;
 (3) nine restatements with one defect each are rejected by the judge; (d), (e), (g) are ACCEPTED by the whole-tensor criterion the older
     tests use (test_gemm_ln_gpu._rel at 8e-3 / 2e-2 on the bf16 333-row case): the gap this suite closes.

The 0.6 of (2) is asserted on every output whose bound is an estimate of fp32 arithmetic: all of them in fp32 except z, and mean / rstd in
bf16. It cannot hold where the bound is the exact size of one event: a bf16-stored output sits within half a bf16 ulp of its fp32 value, and
the worst of thousands of elements reaches 0.9-1.0 of exactly that allowance; z is at most five roundings, each counted, and the worst
element reaches 0.6-0.9 of their sum. Those outputs are held to the judge (<= 1.0); the fp32 cases run the same arithmetic on the same
classes and carry the headroom claim. Figures: fp32 y / mean / rstd / dres / dx stay below 0.27, the column sums below 0.14."""
import numpy as np
import pytest
import torch

import ln_hard_inputs as H
from test_gemm_ln_gpu import _rel

BF16, F32 = torch.bfloat16, torch.float32
SEED, OFFSET, P = 7, 11, 0.1
# name -> (columns, lanes per row, elements per access): 256 lanes = the four waves of the wide kernels
LAYOUTS = {"100/64": (100, 64, 4), "128/16": (128, 16, 8), "192/8": (192, 8, 8), "768/64": (768, 64, 4), "768/32": (768, 32, 8),
           "1024/32": (1024, 32, 8), "2048/64": (2048, 64, 4), "4096/256": (4096, 256, 4)}


# ---------------------------------------------------------------------------------------------- (1) class properties
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cols", [100, 768])
def test_class_properties(dtype, cols):
    rows = 37
    x = H.hard_rows(rows, cols, dtype, 1)
    cls = H.row_classes(rows)
    mean, rstd, _, _, _ = H.ref_stats(x, 1e-5)
    xd = x.double()
    var = ((xd - mean[:, None]) ** 2).mean(-1)
    assert torch.equal(x.float().to(dtype), x) and x.dtype == dtype                      # exact in the storage type
    assert (var[cls == H.CONST] == 0).all() and (xd[cls == H.CONST] == 3.25).all()
    assert (var[cls == H.TINY] < 1e-5 / 5).all() and (var[cls == H.TINY] > 0).all()
    if dtype == F32:
        assert ((mean.abs() * rstd)[cls == H.OFFSET] > 50).all()
    else:
        assert ((mean.abs() * rstd)[cls == H.OFFSET] > 40).all()                            # 64 against sigma ~ 1
    o = xd[cls == H.OUTLIER]
    assert (o[:, 1] == 300).all() and (o[:, cols - 2] == -180).all()
    nc = xd[cls == H.NEARCONST]
    assert ((nc != 5.0).sum(-1) == 1).all() and (nc.amax(-1) == 5 + 2.0 ** -5).all()
    assert (xd[cls == H.BIG].abs().amax(-1) > 2.0 ** 15).all()


@pytest.mark.parametrize("rows", [37, 333])
def test_every_class_in_the_ragged_tail(rows):
    # the last 4 rows are the last workgroup of the one-wave-per-row kernels; over the suite's widths and the two row counts every class
    # lands there, and the last 7 rows (one half-wave workgroup is 8) hold all of them at either count
    assert set(H.row_classes(rows)[-7:].tolist()) == set(range(7))
    tails = set(H.row_classes(37)[-4:].tolist()) | set(H.row_classes(333)[-4:].tolist())
    assert tails == set(range(7)), tails


def test_store_term_is_half_a_bf16_ulp():
    """amendment (i) of ln_hard_inputs: one store to bf16 moves a value by up to half an ulp of its binade, U(bf16) times the binade's closing
    power of two -- up to 2^-8 of the value itself, never more than the term allows, and the term is reached"""
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0, 1.9921875, 2.0 - 2.0 ** -20, 3.0, -0.75, 0.0], dtype=torch.float64)
    assert H.store_term(v, BF16).tolist() == [2.0 ** -8, 2.0 ** -9, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0]
    assert H.store_term(v, F32).abs().max() == 0
    g = torch.Generator().manual_seed(0)
    x = torch.randn(100000, generator=g, dtype=torch.float64) * 2.0 ** torch.randint(-20, 20, (100000,), generator=g)
    ratio = (x.float().bfloat16().double() - x).abs() / H.store_term(x, BF16)
    assert 0.99 < float(ratio.max()) <= 1.0 + 2.0 ** -15          # the fp32 step of the conversion is the only slack
    assert float(((x.float().bfloat16().double() - x).abs() / (H.U_BF16 * x.abs())).max()) > 1.9      # U |ref| alone is half of what a store needs


# ---------------------------------------------------------------------------------------------- (2) the restatement
def _gather(t, lay):
    """[rows, cols] -> [rows, lanes, slots] in the order a lane meets its elements, zero where the lane has no column; and the vector width"""
    cols, L, V = lay
    lane = torch.arange(L)
    if L == 256:
        nvw = -(-(-(-cols // 256)) // 4)
        wave, ln = lane // 64, lane % 64
        base = [((wave * nvw + i) * 64 + ln) * 4 for i in range(nvw)]
    else:
        base = [(i * L + lane) * V for i in range(-(-cols // (L * V)))]
    idx = torch.stack([b + k for b in base for k in range(V)], 1)                 # [lanes, slots]
    ok = idx < cols
    return torch.where(ok, t[:, idx.clamp_max(cols - 1)], torch.zeros((), dtype=t.dtype)), ok, V


def _lane_sum(P, V, by_vector):
    s = torch.zeros_like(P[:, :, 0])
    for i in range(0, P.shape[2], V):
        if by_vector and V == 4:        # ln_fwd_kernel: s += t[0] + t[1] + t[2] + t[3]
            s = s + (((P[:, :, i] + P[:, :, i + 1]) + P[:, :, i + 2]) + P[:, :, i + 3])
        else:
            for k in range(V):
                s = s + P[:, :, i + k]
    return s


def _group_reduce(s):
    L = s.shape[1]
    lane = torch.arange(L)
    o = min(L, 64) // 2
    while o:
        s = s + s[:, lane ^ o]
        o //= 2
    return (s[:, 0] + s[:, 64]) + (s[:, 128] + s[:, 192]) if L == 256 else s[:, 0]


def _row_sum(t, lay, by_vector=False):
    P, _, V = _gather(t, lay)
    return _group_reduce(_lane_sum(P, V, by_vector))


def _ks32(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def emu_fwd(c, eps, lay, keep=None, p=0.0, write_z=True, mut=None, mut_row=0):
    f = lambda t: None if t is None else t.float()
    inv_n = float(np.float32(1.0) / np.float32(c.cols))
    eps32 = float(np.float32(eps))
    t = f(c.x)
    if c.bias is not None:
        t = t + f(c.bias)
    if keep is not None:
        t = torch.where(keep, t * _ks32(p), torch.zeros(()))
    if c.residual is not None:
        t = t + f(c.residual)
    zs = t.to(c.dtype)
    v = zs.float() if (write_z and mut != "c") else t
    mu = _row_sum(v, lay, True) * inv_n
    if mut == "d":
        mu = mu.clone(); mu[mut_row] = mu[mut_row + 1]
    if mut == "a":
        var = _row_sum(v * v, lay) * inv_n - mu * mu
    else:
        P, ok, V = _gather(v, lay)
        d = torch.where(ok, P - mu[:, None, None], torch.zeros(()))
        var = _group_reduce(_lane_sum(d * d, V, False)) * inv_n
    rs = 1.0 / torch.sqrt(var) + eps32 if mut == "b" else 1.0 / torch.sqrt(var + eps32)
    y = (v - mu[:, None]) * rs[:, None]
    if c.gamma is not None:
        y = y * f(c.gamma)
    if c.beta is not None:
        y = y + f(c.beta)
    return (zs if write_z else None), y.to(c.dtype), mu, rs


def emu_finalize(part, dtype, prior=None):
    """colsum_finalize: 1024 partial rows -> one row; thread (ry, cx) adds rows ry + 16 j + 256 it into s_(j % 4)"""
    P = part.reshape(4, 16, 16, -1)
    s = [torch.zeros_like(P[0, 0]) for _ in range(4)]
    for it in range(4):
        for k in range(4):
            for m in range(4):
                s[m] = s[m] + P[it, 4 * k + m]
    red = (s[0] + s[1]) + (s[2] + s[3])
    out = torch.zeros_like(red[0])
    for ry in range(16):
        out = out + red[ry]
    return ((0.0 if prior is None else prior.float()) + out).to(dtype)


def emu_colsum(term, rows_per_block, dtype, prior=None):
    rows, cols = term.shape
    assert rows <= H.PART_BLOCKS * rows_per_block
    pad = torch.zeros((H.PART_BLOCKS * rows_per_block, cols))
    pad[:rows] = term
    blk = pad.reshape(H.PART_BLOCKS, rows_per_block, cols)
    part = torch.zeros((H.PART_BLOCKS, cols))
    for w in range(rows_per_block):
        part = part + blk[:, w]
    return emu_finalize(part, dtype, prior)


def _rows_per_block(lay):
    return 1 if lay[1] == 256 else 4 * (64 // min(lay[1], 64))


def emu_bwd(c, z, mean, rstd, lay, keep=None, p=0.0, mut=None, priors=(None, None, None)):
    f = lambda t: None if t is None else t.float()
    inv_n = float(np.float32(1.0) / np.float32(c.cols))
    mu, rs = mean[:, None], rstd[:, None]
    xh = (f(z) - mu) * rs
    d = f(c.dy)
    gy = d if c.gamma is None else d * f(c.gamma)
    src = d if mut == "f" else gy
    s1 = (_row_sum(src, lay) * inv_n)[:, None]
    s2 = (_row_sum(src * xh, lay) * inv_n)[:, None]
    dz = rs * ((gy - s1) - xh * s2)
    dzi = f(c.dz_in).clone()
    if mut == "g":
        dzi[-1] = 0.0
    dz = dz + dzi
    dx = dz if keep is None else torch.where(keep, dz * _ks32(p), torch.zeros(()))
    n = c.rows - 1 if mut == "e" else c.rows
    rpb = _rows_per_block(lay)
    pri = (None, None, None) if mut == "i" else priors
    sums = [emu_colsum(t[:n], rpb, c.dtype, q) for t, q in zip((d * xh, d, dz if mut == "h" else dx), pri)]
    return dx.to(c.dtype), dz.to(c.dtype), sums[0], sums[1], sums[2]


def _depth(lay, rows):
    L = lay[1]
    return H.colsum_depth("wide", rows) if L == 256 else H.colsum_depth("wave", rows) if L == 64 else H.colsum_depth("half", rows, L)


def _run(lay, dtype, eps, rows=37, mut=None, mut_row=0, priors=False, seed=20):
    """the restatement of the full form on hard rows -> (forward items, backward items, case, outputs)"""
    c = H.make_case(rows, lay[0], dtype, seed=seed)
    keep = H.keep_mask(SEED, OFFSET, rows, lay[0], P)
    fwd = emu_fwd(c, eps, lay, keep, P, mut=mut if mut in ("a", "b", "c", "d") else None, mut_row=mut_row)
    clean = emu_fwd(c, eps, lay, keep, P) if mut is not None else fwd                   # the backward's inputs are never the mutated ones
    pri = tuple(H.small((lay[0],), dtype, 40 + i) for i in range(3)) if priors else (None, None, None)
    bwd = emu_bwd(c, clean[0], clean[2], clean[3], lay, keep, P, mut=mut if mut in ("e", "f", "g", "h", "i") else None, priors=pri)
    fi = H.forward_items(c, fwd, eps, keep, P)
    bi = H.backward_items(c, clean[0], clean[2], clean[3], bwd, _depth(lay, rows), keep, P, priors=pri)
    return fi, bi, c, fwd, bwd


def _headroom(ratios, dtype):
    """below 0.6 wherever the bound estimates fp32 arithmetic (see the module docstring); the judge has held the rest to 1.0"""
    names = [n for n in ratios if n in ("mean", "rstd")] if dtype == BF16 else [n for n in ratios if n != "z"]
    assert all(ratios[n] < 0.6 for n in names), ratios


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_emulation_passes(name, dtype, eps):
    fi, bi, c, _, _ = _run(LAYOUTS[name], dtype, eps, mut=None)
    ratios = H.judge_all(f"emulation {name} {dtype} eps={eps:g}", fi + bi, c.cls)
    _headroom(ratios, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["128/16", "768/64", "4096/256"])
def test_emulation_passes_on_the_classes_themselves(name, dtype):
    """plain LayerNorm (z = x is the class row: variance below eps, constant rows under eps = 1e-12) and the backward fed those rows as z"""
    lay = LAYOUTS[name]
    for eps in (1e-5, 1e-12):
        c = H.make_case(37, lay[0], dtype, seed=30, bias=False, residual=False)
        fwd = emu_fwd(c, eps, lay, write_z=False)
        bwd = emu_bwd(c, c.x, fwd[2], fwd[3], lay)
        items = H.forward_items(c, fwd, eps) + H.backward_items(c, c.x, fwd[2], fwd[3], bwd, _depth(lay, 37))
        ratios = H.judge_all(f"emulation plain {name} {dtype} eps={eps:g}", items, c.cls)
        _headroom(ratios, dtype)


# ---------------------------------------------------------------------------------------------- (3) mutants
def _ratios(items, cls):
    """{output: (largest observed / allowed, rejected?)}"""
    out = {}
    for name, got, ref, bound in items:
        try:
            out[name] = (H.judge(name, got, ref, bound, cls), False)
        except H.JudgeError as e:
            out[name] = (e.worst, True)
    return out


def _old_criterion(items, dtype):
    """the whole-tensor L2 ratios of tests/test_gemm_ln_gpu.py / test_layernorm_dropout_gpu.py::test_fp64_parity"""
    tol_f, tol_b = (3e-6, 2e-5) if dtype == F32 else (8e-3, 2e-2)
    return {name: _rel(got, ref) / (tol_f if name in ("z", "y", "mean", "rstd") else tol_b) for name, got, ref, _ in items}


LAY = LAYOUTS["768/32"]
# (mutant, dtype, rows, outputs the judge must reject; the clean restatement of the same case must pass them)
MUTANTS = [("a", F32, 37, ["rstd", "y"]), ("b", F32, 37, ["rstd", "y"]), ("c", BF16, 37, ["mean", "rstd"]),
           ("d", BF16, 333, ["mean", "y"]), ("e", BF16, 333, ["dgamma", "dbeta", "dbias"]), ("f", F32, 37, ["dres", "dx"]),
           ("g", BF16, 333, ["dres", "dx"]), ("h", F32, 37, ["dbias"]), ("i", F32, 37, ["dgamma", "dbeta", "dbias"])]


@pytest.mark.parametrize("mut,dtype,rows,outputs", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_rejected(mut, dtype, rows, outputs):
    cls = H.row_classes(rows)
    # (d): the last outlier row that has a tiny row behind it takes that row's mean (the two share a wave in the half-wave kernels)
    cand = [r for r in range(rows - 1) if cls[r] == H.OUTLIER and cls[r + 1] == H.TINY]
    fi, bi, c, _, _ = _run(LAY, dtype, 1e-5, rows=rows, mut=mut, mut_row=cand[-1], priors=mut == "i")
    got = _ratios(fi + bi, c.cls)
    clean_f, clean_b, *_ = _run(LAY, dtype, 1e-5, rows=rows, priors=mut == "i")
    clean = _ratios(clean_f + clean_b, c.cls)
    print("MUTANT", mut, {n: f"{v:.3g}" for n, (v, _) in got.items()}, "clean", {n: f"{v:.3g}" for n, (v, _) in clean.items()})
    for name in outputs:
        ratio, rejected = got[name]
        assert rejected and not ratio <= 1.0, (mut, name, ratio)
        assert not clean[name][1], (name, clean[name])
    if rows == 333:
        old = _old_criterion(fi + bi, dtype)
        print("MUTANT", mut, "old criterion, error / tolerance", {n: f"{v:.3g}" for n, v in old.items()})
        assert max(old.values()) < 1.0, "the old whole-tensor criterion was expected to accept this mutant"
