"""GPU: the fused AdamW update and the global grad-norm clip (valor_amd/csrc/optim.hip) against fp64 torch arithmetic on the same
inputs, kernel by kernel on hand-built arenas and through FusedAdamW on a real model arena.

The update is compared as an UPDATE (master after - master before) per element, not as parameters: a relative error on p hides a wrong
lr. Tolerances, from fp32 arithmetic (unit roundoff u = 6e-8):
  * m, v: a handful of roundings of the terms b * m and (1 - b) * g (* g): RTOL_STATE times the sum of the terms' magnitudes;
  * update: the kernel rounds the new master to fp32, so the difference of two fp32 masters is exact only up to one ulp of the larger
    of them (two ulps allowed); on top of that RTOL_STATE of the Adam term (step_size * (|b1 m| + |(1-b1) g|) / denom, i.e. the
    error m carries) plus of the decay term lr * wd * |p|.
A wrong lr / wd, the bias correction of another step, or decay applied before the Adam step miss these bounds by orders of magnitude
(the groups below include lr * wd = 2.5e-2, which moves "decay first" by ~1e-3 against ulps of ~1e-9)."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import lib  # noqa: E402
from valor_amd.kernels import _ptr, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

CH = 1024
B1, B2, EPS = 0.9, 0.98, 1e-6
RTOL_STATE = 1e-5
RTOL_NORM = 2e-5            # fp32 partial sums of up to ~200 sequential terms per thread + two tree levels
# twelve groups: distinct lr / wd, an lr = 0 group, wd = 0 groups, and a large lr * wd
LRS = [1e-3, 2e-3, 0.0, 5e-4, 3e-3, 1.5e-3, 7e-4, 4e-3, 5e-2, 2.5e-3, 8e-4, 1.2e-3]
WDS = [0.01, 0.0, 0.01, 0.1, 0.0, 0.02, 0.05, 0.0, 0.5, 0.01, 0.0, 0.2]


def _dt(dtype):
    return lib.DT_BF16 if dtype == torch.bfloat16 else lib.DT_F32


def _farr(xs):
    return (ctypes.c_float * len(xs))(*xs)


def _ulp32(x):
    """ulp of fp32 values (float64 tensor of magnitudes)"""
    e = torch.frexp(x.abs().float().clamp_min(1e-30))[1].double()
    return torch.ldexp(torch.ones_like(e), (e - 24).to(torch.int32))


class Arena:
    """Hand-built flat arena: tensors of given sizes and groups (-1 = inactive), each starting at a chunk boundary, padding zero."""

    def __init__(self, sizes, groups, dtype, dev, seed, scale_tail=False):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.sizes, self.groups, self.dtype = sizes, groups, dtype
        self.offs, off = [], 0
        for n in sizes:
            self.offs.append(off)
            off += (n + CH - 1) // CH * CH
        self.n, self.nchunks = off, off // CH
        valid = torch.zeros(off, dtype=torch.bool)
        table = torch.full((self.nchunks,), -1, dtype=torch.int8)
        ctens = torch.full((self.nchunks,), -1, dtype=torch.int32)
        for i, (o, n, gr) in enumerate(zip(self.offs, sizes, groups)):
            valid[o:o + n] = True
            table[o // CH:(o + n + CH - 1) // CH] = gr
            ctens[o // CH:(o + n + CH - 1) // CH] = i
        self.valid, self.table, self.chunk_tensor = valid.to(dev), table.to(dev), ctens.to(dev)
        self.active = (table.to(dev).repeat_interleave(CH) >= 0)
        # chunk -> element lr / wd in fp64 (inactive: 0)
        gi = table.long().clamp_min(0).repeat_interleave(CH)
        self.lr = torch.tensor(LRS, dtype=torch.float64)[gi].to(dev)
        self.wd = torch.tensor(WDS, dtype=torch.float64)[gi].to(dev)

        def rnd(std):
            return (torch.randn(off, generator=g) * std).to(dev) * valid.to(dev)

        self.master = rnd(0.05)
        self.m = rnd(1e-3)
        self.v = rnd(1e-3) ** 2 + 1e-8 * valid.to(dev)
        grad = rnd(1e-2)
        if scale_tail:                  # energy in the chunks only later loop iterations and the clamped tail reach
            grad[16384 * CH:] *= 3.0
            grad[(self.nchunks - 1) * CH:] *= 100.0
        self.grad = grad.to(dtype)
        self.param = self.master.to(dtype) if dtype == torch.bfloat16 else None

    def clone_state(self):
        return [None if t is None else t.clone() for t in (self.master, self.m, self.v, self.grad, self.param)]


def _adamw(a, step, gscale=None, zero_grad=1, ngroups=len(LRS), correct_bias=1):
    lib.call("valor_adamw", _stream(), _dt(a.dtype), _ptr(a.master), _ptr(a.m), _ptr(a.v), _ptr(a.grad), _ptr(a.param), _ptr(a.table), a.n,
             _farr(LRS[:ngroups]), _farr(WDS[:ngroups]), ngroups, B1, B2, EPS, step, correct_bias, _ptr(gscale), zero_grad)


def _adamw_counted(a, counts, chunk_bc, gscale=None, zero_grad=1):
    lib.call("valor_adamw_counted", _stream(), _dt(a.dtype), _ptr(a.master), _ptr(a.m), _ptr(a.v), _ptr(a.grad), _ptr(a.param),
             _ptr(a.table), _ptr(a.chunk_tensor), _ptr(counts), counts.numel(), _ptr(chunk_bc), a.n, _farr(LRS), _farr(WDS), len(LRS),
             B1, B2, EPS, 1, _ptr(gscale), zero_grad)


def _norm_clip(a, norm_mul, max_norm, grad=None):
    dev = a.master.device
    partial = torch.empty(1024, dtype=torch.float32, device=dev)
    tn, gs = torch.empty((), dtype=torch.float32, device=dev), torch.empty((), dtype=torch.float32, device=dev)
    lib.call("valor_grad_norm_clip", _stream(), _dt(a.dtype), _ptr(a.grad if grad is None else grad), _ptr(a.table), a.n, norm_mul,
             max_norm, _ptr(partial), _ptr(tn), _ptr(gs))
    torch.cuda.synchronize()
    return float(tn), float(gs)


def _ref_step(master, m, v, grad, gs, lr, wd, step):
    """HF AdamW (optim/adamw.py:76-101) in fp64, per element; step: scalar or per-element tensor. Returns (update, m1, v1, m_terms,
    v_terms, update_terms, p1): the three *_terms are the magnitudes the tolerances are relative to."""
    p, m, v = master.double(), m.double(), v.double()
    g = grad.double() * gs
    m1 = B1 * m + (1 - B1) * g
    v1 = B2 * v + (1 - B2) * g * g
    step = torch.as_tensor(step, dtype=torch.float64, device=p.device)
    bc1, bc2 = 1 - B1 ** step, torch.sqrt(1 - B2 ** step)
    denom = v1.sqrt() + EPS
    step_size = lr * bc2 / bc1
    p1 = p - step_size * m1 / denom
    p1 = torch.where(wd > 0, p1 - lr * wd * p1, p1)
    m_terms = (B1 * m).abs() + ((1 - B1) * g).abs()
    v_terms = B2 * v + (1 - B2) * g * g
    return p1 - p, m1, v1, m_terms, v_terms, step_size * m_terms / denom + lr * wd * p.abs(), p1


def _check_update(before, after, ref, sel, what):
    """before / after: (master, m, v) of the kernel; ref: _ref_step(...) of `before`; sel: bool mask of the elements to compare"""
    upd, m1, v1, m_terms, v_terms, upd_terms, p1 = ref
    got = after[0].double() - before[0].double()
    tol_u = 2 * _ulp32(torch.maximum(before[0].double().abs(), p1.abs())) + RTOL_STATE * upd_terms
    for name, x, y, tol in (("update", got, upd, tol_u), ("exp_avg", after[1].double(), m1, RTOL_STATE * m_terms + 1e-30),
                            ("exp_avg_sq", after[2].double(), v1, RTOL_STATE * v_terms + 1e-30)):
        err = (x - y).abs()
        bad = (err > tol) & sel
        assert not bool(bad.any()), (what, name, int(bad.sum()), float((err / tol)[sel].max()))


def _unchanged(before, after, mask, what):
    for name, b, x in zip(("master", "exp_avg", "exp_avg_sq", "grad", "param"), before, after):
        if b is None:
            continue
        assert torch.equal(b[mask].view(torch.int32 if b.dtype == torch.float32 else torch.int16),
                           x[mask].view(torch.int32 if x.dtype == torch.float32 else torch.int16)), (what, name)


# -------------------------------------------------------------------------------------------------------------------- kernel level

def _layout(kind):
    """(sizes, groups) of the hand-built arenas: every group present, inactive tensors in between, sizes off the chunk grid"""
    if kind == "one":
        return [1000], [3]
    if kind == "odd":               # 37 chunks
        sizes = [1500, 1024, 700, 3000, 2048, 5000, 1, 4096, 2500, 1100, 6000, 900, 3333, 1025]
        groups = [0, 1, -1, 2, 3, 4, 5, -1, 6, 7, 8, 9, 10, 11]
        assert sum((n + CH - 1) // CH for n in sizes) % 2 == 1
        return sizes, groups
    # "large": 40961 chunks -- both kernels' later grid-stride iterations (the update walks 16384 chunks per iteration, the norm kernel
    # 8192 (fp32) / 16384 (bf16)) and an odd count, so the last iteration clamps its tail chunk
    sizes = [1600 * CH + 17] * 24 + [2537 * CH - 17]
    groups = [i % 12 for i in range(24)] + [7]
    groups[5] = groups[13] = -1
    assert sum((n + CH - 1) // CH for n in sizes) == 40961
    return sizes, groups


@pytest.mark.parametrize("kind", ["one", "odd", "large"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_adamw_update_vs_fp64(dev, dtype, kind):
    sizes, groups = _layout(kind)
    a = Arena(sizes, groups, dtype, dev, seed=11, scale_tail=kind == "large")
    step, gs_val = 3, 0.75
    gscale = torch.tensor(gs_val, dtype=torch.float32, device=dev)
    before = a.clone_state()
    ref = _ref_step(a.master, a.m, a.v, a.grad, gs_val, a.lr, a.wd, step)
    _adamw(a, step, gscale)
    torch.cuda.synchronize()
    after = a.clone_state()
    sel = a.active & a.valid
    _check_update(before, after, ref, sel, kind)
    # every group moved (lr = 0 moves only through nothing: group 2's update is exactly zero, its moments still advance)
    lr0 = sel & (a.lr == 0)
    if bool(lr0.any()):
        assert torch.equal(after[0][lr0], before[0][lr0])
    # inactive chunks: bit-unchanged, gradients included
    _unchanged(before, after, ~a.active, "inactive")
    # padding inside an active tensor's last chunk stays zero everywhere
    pad = a.active & ~a.valid
    for t in after:
        if t is not None:
            assert not bool(t[pad].float().abs().sum())
    # active gradients are cleared; bf16 parameters are the masters rounded, bit for bit (FusedAdamW.sync_master's contract)
    assert not bool(after[3][a.active].float().abs().sum())
    if dtype == torch.bfloat16:
        assert torch.equal(after[4].view(torch.int16), after[0].to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_adamw_no_gscale_no_zero_grad_and_nt_modes(dev, dtype):
    """gscale_dev = NULL means a scale of 1; zero_grad = 0 leaves the gradients alone; the four non-temporal modes are bit-identical"""
    sizes, groups = _layout("odd")
    so = lib.load()
    prev = so.valor_adamw_set_nt(-1)
    try:
        outs = []
        for mode in range(4):
            a = Arena(sizes, groups, dtype, dev, seed=12)
            before = a.clone_state()
            ref = _ref_step(a.master, a.m, a.v, a.grad, 1.0, a.lr, a.wd, 1)
            so.valor_adamw_set_nt(mode)
            _adamw(a, 1, None, zero_grad=0)
            torch.cuda.synchronize()
            after = a.clone_state()
            _check_update(before, after, ref, a.active & a.valid, f"nt={mode}")
            assert torch.equal(after[3].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               before[3].view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
            outs.append(after)
        for mode in range(1, 4):
            for x, y in zip(outs[0], outs[mode]):
                if x is not None:
                    assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                                       y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)), mode
    finally:
        so.valor_adamw_set_nt(prev)
    assert so.valor_adamw_set_nt(-1) == prev


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_adamw_counted_per_tensor_steps(dev, dtype):
    """valor_adamw_counted: every tensor's bias correction from its own device count (one launch for tensors at different steps); the
    counts of the active tensors advance, the inactive ones' stay; a skipped step (NaN gscale) advances none"""
    sizes, groups = _layout("odd")
    a = Arena(sizes, groups, dtype, dev, seed=13)
    counts0 = [0, 1, 5, 2, 0, 9, 3, 4, 1, 0, 7, 2, 6, 1]
    counts = torch.tensor(counts0, dtype=torch.int32, device=dev)
    chunk_bc = torch.empty(2 * a.nchunks, dtype=torch.float32, device=dev)
    step_el = (torch.tensor(counts0, dtype=torch.float64, device=dev)[a.chunk_tensor.long().clamp_min(0)] + 1).repeat_interleave(CH)
    gs_val = 0.5
    gscale = torch.tensor(gs_val, dtype=torch.float32, device=dev)
    before = a.clone_state()
    ref = _ref_step(a.master, a.m, a.v, a.grad, gs_val, a.lr, a.wd, step_el)
    _adamw_counted(a, counts, chunk_bc, gscale)
    torch.cuda.synchronize()
    after = a.clone_state()
    _check_update(before, after, ref, a.active & a.valid, "counted")
    _unchanged(before, after, ~a.active, "inactive")
    want = [c + (g >= 0) for c, g in zip(counts0, groups)]
    assert counts.tolist() == want
    # the same update through valor_adamw (host step) for the tensors at one count: bit-identical
    b = Arena(sizes, groups, dtype, dev, seed=13)
    _adamw(b, 3, gscale)                                # count 2 -> step 3: tensors 3 and 11
    torch.cuda.synchronize()
    for i in (3, 11):
        o, n = a.offs[i], sizes[i]
        assert torch.equal(b.master[o:o + n], after[0][o:o + n]) and torch.equal(b.m[o:o + n], after[1][o:o + n])
    # a skipped step: state bit-unchanged, active gradients cleared, counts stay
    a.grad.copy_(before[3])
    nan = torch.tensor(float("nan"), dtype=torch.float32, device=dev)
    state = a.clone_state()
    _adamw_counted(a, counts, chunk_bc, nan)
    torch.cuda.synchronize()
    _unchanged(state[:3] + [None, state[4]], a.clone_state()[:3] + [None, a.param], torch.ones_like(a.active), "skipped")
    assert not bool(a.grad[a.active].float().abs().sum())
    _unchanged([None, None, None, state[3], None], [None, None, None, a.grad, None], ~a.active, "skipped inactive grad")
    assert counts.tolist() == want


@pytest.mark.parametrize("kind", ["one", "odd", "large"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_grad_norm_clip_vs_fp64(dev, dtype, kind):
    sizes, groups = _layout(kind)
    a = Arena(sizes, groups, dtype, dev, seed=14, scale_tail=kind == "large")
    g64 = a.grad.double() * a.active
    ss = float((g64 * g64).sum())
    assert ss > 0
    for norm_mul in (1.0, 0.5, 0.125):
        norm = math.sqrt(ss) * norm_mul
        for max_norm in (-1.0, 0.0, 10.0 * norm, 0.3 * norm):
            tn, gs = _norm_clip(a, norm_mul, max_norm)
            assert abs(tn - norm) <= RTOL_NORM * norm, (norm_mul, max_norm, tn, norm)
            coef = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6))          # torch clip_grad_norm_'s coefficient
            if coef == 1.0:
                assert gs == norm_mul, (max_norm, gs)
            else:
                assert abs(gs - coef * norm_mul) <= RTOL_NORM * coef * norm_mul, (norm_mul, max_norm, gs, coef)
    # an inactive chunk's gradient does not count, however large
    off = [i for i, gr in enumerate(groups) if gr < 0]
    if off:
        o, n = a.offs[off[0]], sizes[off[0]]
        g2 = a.grad.clone()
        g2[o:o + n] = 1e4
        tn, _ = _norm_clip(a, 1.0, -1.0, grad=g2)
        assert abs(tn - math.sqrt(ss)) <= RTOL_NORM * math.sqrt(ss)


@pytest.mark.parametrize("bad", ["inf_first", "nan_later"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_nonfinite_norm_skips_update(dev, dtype, bad):
    """a non-finite gradient: total_norm not finite, gscale NaN, and the update leaves master / m / v / param of every chunk bit-unchanged,
    clears every active gradient chunk and leaves the inactive ones alone"""
    sizes, groups = _layout("odd")
    a = Arena(sizes, groups, dtype, dev, seed=15)
    act_chunks = (a.table >= 0).nonzero().flatten().tolist()
    if bad == "inf_first":
        a.grad[act_chunks[0] * CH + 5] = float("inf")
    else:
        a.grad[act_chunks[len(act_chunks) // 2] * CH + 517] = float("nan")
    tn, gs = _norm_clip(a, 1.0, 5.0)
    assert not math.isfinite(tn) and math.isnan(gs)
    gscale = torch.tensor(gs, dtype=torch.float32, device=dev)
    before = a.clone_state()
    _adamw(a, 2, gscale)
    torch.cuda.synchronize()
    after = a.clone_state()
    everything = torch.ones_like(a.active)
    _unchanged(before[:3] + [None, before[4]], after[:3] + [None, after[4]], everything, "skipped")
    assert not bool(after[3][a.active].float().abs().sum())
    _unchanged([None] * 3 + [before[3], None], [None] * 3 + [after[3], None], ~a.active, "inactive grad")


# ---------------------------------------------------------------------------------------------------------------- optimizer level

def _model_opt(dtype, dev):
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    from valor_amd.optim import FusedAdamW
    spec = synth.tiny_spec()
    model = VALOR({"dropout": 0.0, "drop_path_rate": 0.0}, spec=spec, dtype=dtype, device=dev)
    model.load_state_dict(synth.make_state_dict(spec, seed=21), strict=True)
    opt = FusedAdamW(model, dict(learning_rate=1e-3, weight_decay=0.01, betas=[B1, B2]))
    for i, g in enumerate(opt.param_groups):        # ten distinct lrs, decay on the even groups
        g["lr"], g["weight_decay"] = 1e-3 * (1 + 0.37 * i), (0.05 if i % 2 == 0 else 0.0)
    return model, opt


def _grads(arena, seed, bad=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = torch.zeros(arena.numel, dtype=torch.float32)
    for name, (o, n, _) in arena.offsets.items():
        out[o:o + n] = torch.randn(n, generator=g) * 1e-2
    if bad is not None:
        o, n, _ = arena.offsets[bad]
        out[o + n // 2] = float("nan")
    return out.to(arena.dtype).to(arena.device)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_fused_adamw_mixed_step_counts_vs_fp64(dev, dtype):
    """three steps with different active sets: steps 2 and 3 update tensors at different Adam steps in one call; every tensor is
    compared with fp64 arithmetic at its own step count, under a clipping global norm"""
    model, opt = _model_opt(dtype, dev)
    a = opt.arena
    names = list(a.offsets)
    sets = [[n for i, n in enumerate(names) if i % 3 != 1], [n for i, n in enumerate(names) if i % 4 != 2], names]
    count = {n: 0 for n in names}
    for s, active in enumerate(sets):
        a.grad.copy_(_grads(a, 100 + s))
        grad = a.grad.clone()
        before = [opt.master.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]
        act = torch.zeros(a.numel, dtype=torch.bool, device=dev)
        lr = torch.zeros(a.numel, dtype=torch.float64, device=dev)
        wd = torch.zeros_like(lr)
        step = torch.ones_like(lr)
        for n in active:
            o, k, _ = a.offsets[n]
            act[o:o + k] = True
            gr = opt.param_groups[a.groups[n]]
            lr[o:o + k], wd[o:o + k], step[o:o + k] = gr["lr"], gr["weight_decay"], count[n] + 1
        norm = float((grad.double() * act).norm())
        max_norm = 0.5 * norm
        opt.step(active_names=set(active), max_grad_norm=max_norm)
        torch.cuda.synchronize()
        assert abs(float(opt.total_norm) - norm) <= RTOL_NORM * norm
        gs = float(opt.gscale)
        assert abs(gs - max_norm / (norm + 1e-6)) <= RTOL_NORM * gs
        ref = _ref_step(before[0], before[1], before[2], grad, gs, lr, wd, step)
        after = [opt.master, opt.exp_avg, opt.exp_avg_sq]
        _check_update(before, after, ref, act, f"step {s + 1}")
        for n in active:
            count[n] += 1
        # inactive tensors: untouched, their gradients included
        idle = ~act
        for b, x in zip(before + [grad], after + [a.grad]):
            assert torch.equal(b[idle], x[idle])
        assert opt.steps == count
        if opt.separate_master:
            assert torch.equal(a.flat.view(torch.int16), opt.master.to(torch.bfloat16).view(torch.int16))
    assert len({c for c in count.values()}) > 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_skipped_step_does_not_advance_the_count(dev, dtype):
    """run A sees gradients [g1, g_nan, g2], run B [g1, g2]: the NaN step is skipped (apex amp's skip_step for the reference: AdamW's
    state['step'] += 1 never runs), so A ends bit-identical to B and both count 2 steps"""
    runs = {}
    for run, seq in (("A", [(1, None), (2, "nan"), (3, None)]), ("B", [(1, None), (3, None)])):
        model, opt = _model_opt(dtype, dev)
        a = opt.arena
        victim = list(a.offsets)[len(a.offsets) // 2]
        for seed, bad in seq:
            a.grad.copy_(_grads(a, 200 + seed, bad=victim if bad else None))
            opt.step(max_grad_norm=1.0)
            if bad:
                torch.cuda.synchronize()
                assert not math.isfinite(float(opt.total_norm))
                assert not bool(a.grad.float().abs().sum())        # the skipped step still clears the gradients
        torch.cuda.synchronize()
        runs[run] = (model, opt)
    (ma, oa), (mb, ob) = runs["A"], runs["B"]
    for x, y in ((oa.master, ob.master), (oa.exp_avg, ob.exp_avg), (oa.exp_avg_sq, ob.exp_avg_sq), (oa.arena.flat, ob.arena.flat)):
        assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                           y.view(torch.int32 if y.dtype == torch.float32 else torch.int16))
    assert set(oa.steps.values()) == {2} and oa.steps == ob.steps
    sd = oa.state_dict()
    assert len(sd["state"]) == len(oa.arena.offsets) and {st["step"] for st in sd["state"].values()} == {2}
    rsd = oa.reference_state_dict()
    assert rsd["state"] and {st["step"] for st in rsd["state"].values()} == {2}
    # the counts survive a round trip through both checkpoint formats (written back to the device)
    for load, blob in (("load_state_dict", sd), ("load_reference_state_dict", rsd)):
        _, o2 = _model_opt(dtype, dev)
        getattr(o2, load)(blob)
        assert o2.steps == oa.steps, load


def test_adamw_counted_bias_correction_equals_the_host_arithmetic(dev):
    """the device computes (bc1, bc2_sqrt) of step count + 1 exactly as valor_adamw's host code did (double pow, rounded to fp32):
    bit for bit over the first 4096 steps, so moving the count to the device changes no update"""
    import struct
    n = 4096
    a = Arena([CH] * n, [i % 12 for i in range(n)], torch.float32, dev, seed=16)
    counts = torch.arange(n, dtype=torch.int32, device=dev)
    chunk_bc = torch.empty(2 * n, dtype=torch.float32, device=dev)
    _adamw_counted(a, counts, chunk_bc)
    torch.cuda.synchronize()
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]
    b1, b2 = f32(B1), f32(B2)
    want = []
    for s in range(1, n + 1):
        want += [f32(1.0 - math.pow(b1, s)), f32(math.sqrt(1.0 - math.pow(b2, s)))]
    assert chunk_bc.cpu().tolist() == want
    assert torch.equal(counts.cpu(), torch.arange(1, n + 1, dtype=torch.int32))
