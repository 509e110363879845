"""The training diagnostics on the device: valor_arena_grad_stats / valor_arena_update_stats against their fp64 restatement
(diagnostics.stats_host) on a hand-built arena whose padding is NaN everywhere, then Diagnostics inside the optimizer, the engine and the
trainer: it does not perturb training, it agrees with the gradients, it names the tensor that went non-finite, `every` holds the tables
in between, the group rows are logged and survive an exact resume, and it adds no synchronisation.

Tolerances: g_absmax and the counts are exact. A sum of squares is within 1e-5 relative of fp64: the kernels' fp32 part is one chunk's
partial (<= 16 fused multiply-adds in a lane and six butterfly levels, below 23 ulp = 1.4e-6 for non-negative terms), everything above a
chunk is summed in fp64 and rounded once per stored row (include/valor_hip.h); norms and ratios, square roots of those, within 1e-5 too.
Engine setup: that of tests/test_train_gpu.py (synth.tiny_spec(), batch 2, 2 frames, 1 audio slice, txt_len 32, bf16)."""
import ctypes
import gc
import os
import random
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CHUNK = 1024
NUMEL = [1, 1023, 1024, 1025, 3079, 4096]
GROUP = [0, 1, 2, 0, 1, 2]
SCALE = [1e-6, 1e-3, 1.0, 10.0, 1e3, 1e-2]
INACTIVE = 2                                  # the 1024-element tensor
NGROUPS, NORM_MUL, EPS = 3, 0.25, 1e-6
LR = [1e-3, 5e-7, 0.0]
RTOL = 1e-5
F = {k: i for i, k in enumerate(("g_sumsq", "g_absmax", "g_nonfinite", "g_norm", "w_sumsq", "u_sumsq", "w_norm", "u_ratio"))}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _layout(inactive=(INACTIVE,)):
    nch = [(n + CHUNK - 1) // CHUNK for n in NUMEL]
    first = np.concatenate([[0], np.cumsum(nch)[:-1]]).astype(int)
    ct = np.repeat(np.arange(len(NUMEL)), nch).astype(np.int32)
    cg = np.array([-1 if t in inactive else GROUP[t] for t in ct], dtype=np.int8)
    return first, ct, cg, int(sum(nch))


def _arena(seed, kind="normal"):
    """a flat fp32 host array laid out like the arena: tensor t = normal * SCALE[t] ('positive': uniform(0.01, 1) * SCALE[t]^2),
    NaN in every pad element"""
    rng = np.random.default_rng(seed)
    first, _, _, nchunks = _layout()
    a = np.full(nchunks * CHUNK, np.nan, dtype=np.float32)
    for t, n in enumerate(NUMEL):
        o = first[t] * CHUNK
        a[o:o + n] = rng.standard_normal(n) * SCALE[t] if kind == "normal" else rng.uniform(0.01, 1.0, n) * SCALE[t] ** 2
    return a


class Case:
    """device tables of one call and the host copies stats_host reads (a bf16 arena's host copy holds the rounded values)"""

    def __init__(self, dev, dtype, grad_host, inactive=(INACTIVE,), scratch_fill=float("nan")):
        from valor_amd import kernels
        self.dev, self.first, ct, cg, self.nchunks = dev, *_layout(inactive)
        self.ct_h, self.cg_h = ct, cg
        self.grad = torch.from_numpy(grad_host).to(dev).to(dtype)
        self.grad_h = self.grad.float().cpu().numpy()
        self.ct, self.cg = torch.from_numpy(ct).to(dev), torch.from_numpy(cg).to(dev)
        self.numel = torch.tensor(NUMEL, dtype=torch.int64, device=dev)
        self.scratch = torch.full((kernels.stats_scratch_floats(self.nchunks * CHUNK, len(NUMEL)),), scratch_fill, device=dev)
        self.ts = torch.zeros((len(NUMEL), 8), device=dev)
        self.gs = torch.zeros((NGROUPS, 8), device=dev)

    def run_grad(self):
        from valor_amd import kernels
        kernels.arena_grad_stats(self.grad, self.cg, self.ct, self.numel, NORM_MUL, self.scratch, self.ts, self.gs)
        return self.ts.cpu().numpy(), self.gs.cpu().numpy()

    def host(self, **kw):
        from valor_amd.diagnostics import stats_host
        return stats_host(self.cg_h, self.ct_h, NUMEL, NGROUPS, norm_mul=NORM_MUL, **kw)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err[want == 0] = np.abs(got[want == 0])
    print(f"{what}: max relative error {err.max():.3e}")
    assert (err <= RTOL).all(), (what, got.tolist(), want.tolist())


def _check_grad_fields(got, want, what):
    for k in ("g_absmax", "g_nonfinite"):
        assert got[:, F[k]].tolist() == want[:, F[k]].astype(np.float32).tolist(), (what, k)
    _close(got[:, F["g_sumsq"]], want[:, F["g_sumsq"]], what + " g_sumsq")
    _close(got[:, F["g_norm"]], want[:, F["g_norm"]], what + " g_norm")


DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float32, id="fp32")]


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_stats_against_fp64(dev, dtype):
    """six tensors of 1 .. 4096 elements on 13 chunks, three groups, the 1024-element tensor inactive, NaN behind every tail"""
    c = Case(dev, dtype, _arena(1))
    ts, gs = c.run_grad()
    want_t, want_g = c.host(grad=c.grad_h)
    assert np.isfinite(ts).all() and np.isfinite(gs).all()                       # no pad element reached a statistic
    _check_grad_fields(ts, want_t, "tensor")
    _check_grad_fields(gs, want_g, "group")
    assert not ts[INACTIVE].any() and (ts[[t for t in range(6) if t != INACTIVE], 0] > 0).all()
    assert not ts[:, 4:].any() and not gs[:, 4:].any()                           # the other call's fields were left alone
    assert want_g[2, 0] == want_t[5, 0]                                          # group 2 is the 4096-element tensor alone


@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_stats_non_finite_placement(dev, dtype):
    """NaN in the only element of the 1-element tensor, +inf at element 0 and -inf at element n - 1 of the 1023-element tensor, NaN at
    element 1024 of the 1025-element tensor (the single element of its second chunk): exact counts per tensor and group, sums and maxima
    those of the data with the planted elements removed"""
    first, _, _, _ = _layout()
    clean = _arena(2)
    planted, removed = clean.copy(), clean.copy()
    for t, e, v in ((0, 0, np.nan), (1, 0, np.inf), (1, NUMEL[1] - 1, -np.inf), (3, 1024, np.nan)):
        planted[first[t] * CHUNK + e] = v
        removed[first[t] * CHUNK + e] = 0.0
    c = Case(dev, dtype, planted)
    ts, gs = c.run_grad()
    assert ts[:, F["g_nonfinite"]].tolist() == [1.0, 2.0, 0.0, 1.0, 0.0, 0.0] and gs[:, F["g_nonfinite"]].tolist() == [2.0, 2.0, 0.0]
    r = Case(dev, dtype, removed)
    want_t, want_g = r.host(grad=r.grad_h)
    assert ts[0, :4].tolist() == [0.0, 0.0, 1.0, 0.0]                            # nothing finite is left of the 1-element tensor
    for got, want, what in ((ts, want_t, "tensor"), (gs, want_g, "group")):
        assert got[:, F["g_absmax"]].tolist() == want[:, F["g_absmax"]].astype(np.float32).tolist(), what
        _close(got[:, F["g_sumsq"]], want[:, F["g_sumsq"]], what + " g_sumsq")
        _close(got[:, F["g_norm"]], want[:, F["g_norm"]], what + " g_norm")
    # and the restatement sees the planted data the same way
    also_t, also_g = c.host(grad=c.grad_h)
    _check_grad_fields(ts, also_t, "tensor, planted")
    _check_grad_fields(gs, also_g, "group, planted")


@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_stats_are_deterministic(dev, dtype):
    """two calls (different garbage in the scratch) give the same bits; with the 3079-element tensor inactive as well, the rows of the
    tensors that are active in both calls keep their bits"""
    g = _arena(3)
    a, b = Case(dev, dtype, g), Case(dev, dtype, g, scratch_fill=123.0)
    a.run_grad(), b.run_grad()
    a.run_grad()
    assert torch.equal(_bits(a.ts), _bits(b.ts)) and torch.equal(_bits(a.gs), _bits(b.gs))
    fewer = Case(dev, dtype, g, inactive=(INACTIVE, 4))
    fewer.run_grad()
    both = [0, 1, 3, 5]
    assert torch.equal(_bits(fewer.ts[both]), _bits(a.ts[both])) and not fewer.ts[4].any() and a.ts[4].any()
    assert torch.equal(_bits(fewer.gs[[0, 2]]), _bits(a.gs[[0, 2]])) and not torch.equal(_bits(fewer.gs[1]), _bits(a.gs[1]))


def _update_case(dev):
    """random weights and first moments, positive second moments, per-tensor step counts 1, 2, 1000: chunk_bc as adamw_bc_kernel leaves it"""
    c = Case(dev, torch.float32, _arena(4))
    c.w_h, c.m_h, c.v_h = _arena(5), _arena(6), _arena(7, "positive")
    steps = [1, 2, 1000, 1, 2, 1000]
    bc = np.array([[np.float32(1.0 - 0.9 ** s), np.float32(np.sqrt(1.0 - 0.98 ** s))] for s in steps], dtype=np.float32)
    c.bc_h = bc[c.ct_h]
    c.w, c.m, c.v, c.bc = (torch.from_numpy(x).to(dev) for x in (c.w_h, c.m_h, c.v_h, c.bc_h.reshape(-1)))
    return c


def test_update_stats_against_fp64_and_skipped_step(dev):
    from valor_amd import kernels
    c = _update_case(dev)
    c.run_grad()
    before = c.ts[:, :4].clone()
    gscale = torch.tensor(0.37, device=dev)
    kernels.arena_update_stats(c.w, c.m, c.v, c.cg, c.ct, c.bc, c.numel, LR, EPS, gscale, c.scratch, c.ts, c.gs)
    ts, gs = c.ts.cpu().numpy(), c.gs.cpu().numpy()
    assert torch.equal(_bits(c.ts[:, :4]), _bits(before))                        # the gradient fields were left alone
    want_t, want_g = c.host(master=c.w_h, exp_avg=c.m_h, exp_avg_sq=c.v_h, chunk_bc=c.bc_h, lr=LR, eps=EPS)
    assert np.isfinite(ts).all() and np.isfinite(gs).all()
    for got, want, what in ((ts, want_t, "tensor"), (gs, want_g, "group")):
        for k in ("w_sumsq", "u_sumsq", "w_norm", "u_ratio"):
            _close(got[:, F[k]], want[:, F[k]], f"{what} {k}")
    assert not ts[INACTIVE].any()
    assert (ts[[0, 1, 3, 4], F["u_ratio"]] > 0).all() and ts[5, F["u_ratio"]] == 0 and gs[2, F["u_ratio"]] == 0      # group 2: lr 0
    assert ts[5, F["w_norm"]] > 0
    # the bias corrections differ per tensor: the 1-step and the 1000-step tensor of a group would swap their u_sumsq otherwise
    assert want_t[0, F["u_sumsq"]] != want_t[3, F["u_sumsq"]]
    # a skipped step: fields 5 and 7 exactly zero in every row, 4 and 6 unchanged
    for bad in (float("nan"), float("inf")):
        gscale.fill_(bad)
        kernels.arena_update_stats(c.w, c.m, c.v, c.cg, c.ct, c.bc, c.numel, LR, EPS, gscale, c.scratch, c.ts, c.gs)
        for got, ref in ((c.ts.cpu(), ts), (c.gs.cpu(), gs)):
            assert not got[:, [5, 7]].any()
            assert torch.equal(_bits(got[:, [4, 6]]), _bits(torch.from_numpy(ref[:, [4, 6]])))


def test_stats_kernels_refuse_bad_arguments_on_the_device(dev):
    """every refusal returns VALOR_ERR_ARG and launches nothing: the output tables keep their sentinel"""
    from valor_amd import lib
    from valor_amd.kernels import _stream
    so = lib.load()
    c = _update_case(dev)
    c.ts.fill_(7.0), c.gs.fill_(7.0)
    gscale = torch.ones((), device=dev)
    lr = (ctypes.c_float * NGROUPS)(*LR)
    n = c.nchunks * CHUNK
    p = lambda t: t.data_ptr()

    def grad(n=n, ntensors=6, ngroups=NGROUPS, dtype=1, **kw):
        a = dict(grad=p(c.grad), cg=p(c.cg), ct=p(c.ct), numel=p(c.numel), scratch=p(c.scratch), ts=p(c.ts), gs=p(c.gs))
        a.update(kw)
        return so.valor_arena_grad_stats(_stream(), dtype, a["grad"], a["cg"], a["ct"], a["numel"], ntensors, n, ngroups, 1.0, a["scratch"],
                                         a["ts"], a["gs"])

    def upd(n=n, ntensors=6, ngroups=NGROUPS, lr_=lr, **kw):
        a = dict(master=p(c.w), m=p(c.m), v=p(c.v), cg=p(c.cg), ct=p(c.ct), bc=p(c.bc), numel=p(c.numel), gscale=p(gscale), scratch=p(c.scratch),
                 ts=p(c.ts), gs=p(c.gs))
        a.update(kw)
        return so.valor_arena_update_stats(_stream(), a["master"], a["m"], a["v"], a["cg"], a["ct"], a["bc"], a["numel"], ntensors, n, lr_,
                                           ngroups, EPS, a["gscale"], a["scratch"], a["ts"], a["gs"])

    for f, ptrs in ((grad, ("grad", "cg", "ct", "numel", "scratch", "ts", "gs")),
                    (upd, ("master", "m", "v", "cg", "ct", "bc", "numel", "scratch", "ts", "gs"))):
        assert f(n=n - 24) == -1 and f(n=n + 1) == -1
        assert f(ntensors=0) == -1 and f(ngroups=0) == -1 and f(ngroups=17) == -1
        for k in ptrs:
            assert f(**{k: None}) == -1, k
        for k in ("scratch", "ts", "gs"):
            assert f(**{k: p(getattr(c, k)) + 4}) == -1, k
        assert f(ct=p(c.ct) + 2) == -1 and f(numel=p(c.numel) + 4) == -1
        assert f(n=0) == 0
    assert grad(dtype=5) == -1 and grad(grad=p(c.grad) + 4) == -1
    assert upd(master=p(c.w) + 4) == -1 and upd(bc=p(c.bc) + 4) == -1 and upd(lr_=None) == -1
    torch.cuda.synchronize()
    assert bool((c.ts == 7.0).all()) and bool((c.gs == 7.0).all())
    assert grad() == 0 and upd() == 0                                            # the same arguments, unbroken, go through
    torch.cuda.synchronize()
    assert not bool((c.ts == 7.0).any()) and not bool((c.gs == 7.0).any())


# ------------------------------------------------------------------------------------------------------------------ engine and trainer
TASK_A = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
TASK_B = "pt_contra%tv_mlm%tv"


@pytest.fixture(autouse=True)
def rng_modes(dev):
    from valor_amd import ops
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    gc.collect()


class Sampler:
    def __init__(self):
        self.epoch = 0

    def set_epoch(self, e):
        self.epoch = e


class SynthLoader:
    def __init__(self, tag, n, seed0):
        self.tag, self.n, self.seed0, self.sampler = tag, n, seed0, Sampler()

    def __iter__(self):
        from valor_amd import synth
        e = self.sampler.epoch
        for i in range(self.n):
            b = synth.make_batch(synth.tiny_spec(), batch=2, frames=2, audio_slices=1, txt_len=32, seed=self.seed0 + 100 * e + i)
            b["ids"] = [f"{self.tag}{e}.{i}.{j}" for j in range(2)]
            yield b


def _loaders():
    from valor_amd.train import MetaLoader
    return MetaLoader({TASK_A + "--dsetA": SynthLoader("a", 3, 10), TASK_B + "--dsetB": SynthLoader("b", 2, 500)}, seed=4)


def _opts(steps, **kw):
    return SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-4, clip_lr_text=1e-4, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=steps, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0, **kw)


def _build(dev, weight_seed, opts, graphs=True, new_params=()):
    from valor_amd import synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=weight_seed, w_std=0.05)
    model = VALOR({"dropout": 0.1, "drop_path_rate": 0.0, "token_masker": "host", "seed": 7}, spec=spec, dtype=torch.bfloat16, device=dev)
    model.load_state_dict(sd, strict=True)
    eng = TrainEngine(model, opts, manage_gc=False, graphs=graphs)
    eng.optimizer.init_master_from(sd)
    return model, eng


def _seed_run(seed):
    from valor_amd import ops
    ops.DropoutState.reset(seed)
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    torch.manual_seed(seed + 3)


def _state(eng):
    opt = eng.optimizer
    return {"flat": eng.model.arena.flat.detach().clone(), "master": opt.master.clone(), "exp_avg": opt.exp_avg.clone(),
            "exp_avg_sq": opt.exp_avg_sq.clone(), "steps": opt.steps, "global_step": eng.global_step}


def _same_state(got, want, what):
    for k in ("flat", "master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
    assert got["steps"] == want["steps"] and got["global_step"] == want["global_step"], what


def _teardown(model, eng):
    from valor_amd import decode
    torch.cuda.synchronize()
    model.enable_graphs(False)
    decode.release_sessions(model)
    eng.close()


def _to_dev(batch, dev):
    b = dict(batch)
    b["video_pixels"], b["audio_spectrograms"] = b["video_pixels"].to(dev), b["audio_spectrograms"].to(dev)
    return b


def _batches(dev, n):
    return [(name, _to_dev(b, dev)) for name, b in (x for _, x in zip(range(n), iter(_loaders())))]


def _run_steps(dev, n, level=None, every=1, each=None):
    from valor_amd.diagnostics import Diagnostics
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(8))
    diag = None
    if level is not None:
        diag = eng.diagnostics = Diagnostics(eng.optimizer, level=level, every=every)
    for i, (name, b) in enumerate(_batches(dev, n)):
        eng.train_step(b, name.split("--")[0])
        if each is not None:
            each(i, eng, diag)
    st = _state(eng)
    _teardown(model, eng)
    return st, diag


def test_diagnostics_do_not_perturb_training(dev):
    """four train_steps with Diagnostics(level='full') and the same four steps without: parameters, masters, both moments and the step
    counts are equal to the bit"""
    want, _ = _run_steps(dev, 4)
    got, diag = _run_steps(dev, 4, level="full")
    _same_state(got, want, "with diagnostics")
    assert diag.step_index == 4 and diag.table_step == 3 and bool(diag.group_stats[:, F["g_norm"]].any())


def test_every_two_holds_the_tables_in_between(dev):
    seen = []
    _run_steps(dev, 4, level="full", every=2, each=lambda i, eng, d: seen.append((d.fresh, d.table_step, _bits(d.group_stats), _bits(d.tensor_stats))))
    assert [s[:2] for s in seen] == [(True, 0), (False, 0), (True, 2), (False, 2)]
    assert torch.equal(seen[0][2], seen[1][2]) and torch.equal(seen[0][3], seen[1][3])
    assert torch.equal(seen[2][2], seen[3][2]) and torch.equal(seen[2][3], seen[3][3])
    assert not torch.equal(seen[1][2], seen[2][2]) and not torch.equal(seen[1][3], seen[2][3])


def _hand_step(dev, poison=False):
    """forward, backward, optimizer.step by hand (tests/test_model_gpu.py's pattern); returns what the checks need"""
    from valor_amd.diagnostics import Diagnostics
    from valor_amd.optim import get_lr_sched
    _seed_run(77)
    opts = _opts(8)
    model, eng = _build(dev, 3, opts, graphs=False)
    opt, a = eng.optimizer, model.arena
    diag = Diagnostics(opt, level="full")
    out = {"diag": diag, "names": list(a.offsets), "offsets": dict(a.offsets), "groups": dict(a.groups)}
    from valor_amd import synth
    mk = lambda seed: _to_dev(synth.make_batch(synth.tiny_spec(), batch=2, frames=2, audio_slices=1, txt_len=32, seed=seed), dev)
    for i, (task, b) in enumerate(((TASK_A, mk(10)), (TASK_B, mk(500)))):        # the second step leaves the audio tower without gradients
        eng.reducer.reset_task(task)
        eng.reducer.prepare_backward(defer=True)
        model.train()
        loss = sum(model(b, task=task, compute_loss=True).values())
        loss.backward()
        touched = set(eng.reducer.touched)
        for g in opt.param_groups:
            g["lr"] = g["init_lr"] * get_lr_sched(i + 1, opts)
        if poison and i == 1:
            out["victim"] = sorted(touched)[len(touched) // 2]
            a.params[out["victim"]].grad.view(-1)[0] = float("inf")          # a numeric value in the arena, nothing else
        out.update(grad=a.grad.float().cpu(), touched=touched, steps_before=opt.steps, lr=[g["lr"] for g in opt.param_groups])
        opt.step(active_names=touched, max_grad_norm=5.0, world_size=1, diagnostics=diag)
    out.update(master=opt.master.cpu(), total_norm=float(opt.total_norm), gscale=float(opt.gscale), steps_after=opt.steps,
               ts=diag.tensor_stats.cpu().numpy().astype(np.float64), gs=diag.group_stats.cpu().numpy().astype(np.float64))
    out["table"] = diag.flush()[-1]
    _teardown(model, eng)
    return out


def test_diagnostics_agree_with_the_gradients(dev):
    """the second of two hand-written steps: per-tensor g_norm is the fp64 norm of the tensor's slice of the gradient arena as it stood
    in front of the step, the groups' sums of squares give optimizer.total_norm, w_norm is the norm of the post-step master slice, a group
    moves (u_ratio > 0) iff it has an active tensor and a learning rate"""
    r = _hand_step(dev)
    ts, gs = r["ts"], r["gs"]
    active = [n in r["touched"] for n in r["names"]]
    assert any(active) and not all(active)
    for i, n in enumerate(r["names"]):
        o, k, _ = r["offsets"][n]
        if not active[i]:
            assert not ts[i].any(), n
            continue
        want_g = float(r["grad"][o:o + k].double().norm())
        want_w = float(r["master"][o:o + k].double().norm())
        assert abs(ts[i, F["g_norm"]] - want_g) <= RTOL * want_g, (n, ts[i, F["g_norm"]], want_g)
        assert abs(ts[i, F["w_norm"]] - want_w) <= RTOL * want_w, (n, ts[i, F["w_norm"]], want_w)
        assert ts[i, F["g_nonfinite"]] == 0
    total = float(np.sqrt(gs[:, F["g_sumsq"]].sum()))
    print(f"total norm: optimizer {r['total_norm']:.9g}, from the group rows {total:.9g}")
    assert abs(total - r["total_norm"]) <= RTOL * r["total_norm"] and r["total_norm"] > 0
    has = [any(active[i] and r["groups"][n] == g for i, n in enumerate(r["names"])) for g in range(10)]
    assert sum(has) >= 2
    for g in range(10):
        if has[g] and r["lr"][g] > 0:
            assert gs[g, F["u_ratio"]] > 0 and gs[g, F["w_norm"]] > 0, g
        else:
            assert gs[g, F["u_ratio"]] == 0, g
    assert r["lr"][2] == 0 and r["lr"][3] == 0                                   # new_lr = 0: the `new` groups do not move
    # what flush() delivered is the table
    assert r["table"].names == r["names"] and np.array_equal(r["table"].table, ts) and r["table"].nonfinite_tensors() == []
    top = r["table"].by_module(1)
    assert abs(np.sqrt(sum(v["g_sumsq"] for v in top.values())) - total) <= 1e-6 * total        # fp32 tensor rows against fp32 group rows


def test_diagnostics_name_the_tensor_that_went_non_finite(dev):
    """inf in one element of one tensor's gradient: the step is skipped (the step counts stay), nonfinite_tensors() names exactly that
    tensor, u_sumsq is zero everywhere"""
    r = _hand_step(dev, poison=True)
    assert r["gscale"] != r["gscale"] and r["steps_after"] == r["steps_before"] and r["victim"] in r["touched"]
    assert r["table"].nonfinite_tensors() == [r["victim"]]
    i = r["names"].index(r["victim"])
    assert r["ts"][i, F["g_nonfinite"]] == 1.0 and r["gs"][r["groups"][r["victim"]], F["g_nonfinite"]] == 1.0
    assert r["gs"][:, F["g_nonfinite"]].sum() == 1.0
    assert not r["ts"][:, F["u_sumsq"]].any() and not r["gs"][:, F["u_sumsq"]].any() and not r["gs"][:, F["u_ratio"]].any()
    assert r["ts"][:, F["w_sumsq"]].any() and np.isfinite(r["ts"]).all()


def test_fit_logs_the_group_rows_and_resumes_exactly(dev, tmp_path):
    """six fit steps with diagnostics from the options: the sink's records carry the ten grad_norm/<group> keys; fit to the checkpoint
    at step 3, killed, resumed in a fresh process state: parameters, masters, moments, step counts and the meter table -- group rows
    included -- equal the uninterrupted run's to the bit"""
    from valor_amd import checkpoint
    from valor_amd.diagnostics import GROUP_NAMES
    from valor_amd.train import Trainer, trainer_file
    opts = lambda: _opts(6, valid_steps=4, diag_level="grad")
    _seed_run(77)
    model, eng = _build(dev, 3, opts())
    logged = []
    tr = Trainer(eng, _loaders(), output_dir=str(tmp_path / "full"), log_fn=lambda s, sc: logged.append((s, sc)), log_every=1)
    out = tr.fit()
    assert out["checkpoints"] == [3] and out["global_step"] == 6 and tr.diagnostics is eng.diagnostics is not None
    rows = [sc for _, sc in logged if "grad_norm" in sc]
    assert rows and all(f"grad_norm/{g}" in sc and f"grad_absmax/{g}" in sc for sc in rows for g in GROUP_NAMES)
    assert not any(k.startswith("update_ratio/") for sc in rows for k in sc)     # level 'grad'
    last = out["meter"]
    assert last["grad_norm/basic_decay"]["count"] == 6 and last["grad_norm/basic_decay"]["last"] > 0
    assert last["grad_norm/new_decay"]["max"] >= 0 and not any("nonfinite_tensors" in sc for _, sc in logged)
    want, want_table, want_names = _state(eng), tr.meter.table[:len(tr.meter.names)].clone(), list(tr.meter.names)
    _teardown(model, eng)
    del model, eng, tr

    class Killed(Exception):
        pass
    _seed_run(77)
    model, eng = _build(dev, 3, opts())
    inner = eng.train_step

    def dies_after_three(batch, task, accum_steps=1):
        if eng.global_step == 3:
            raise Killed()
        return inner(batch, task, accum_steps=accum_steps)
    eng.train_step = dies_after_three
    run = str(tmp_path / "run")
    with pytest.raises(Killed):
        Trainer(eng, _loaders(), output_dir=run, log_fn=lambda *a: None).fit()
    _teardown(model, eng)
    assert checkpoint.latest_step(run) == 3 and os.path.exists(trainer_file(run, 3))
    del model, eng
    _seed_run(4000)
    model, eng = _build(dev, 11, opts())
    tr = Trainer(eng, _loaders(), output_dir=run, log_fn=lambda *a: None)
    assert tr.fit(resume=True)["global_step"] == 6
    _same_state(_state(eng), want, "resumed, step 6")
    assert tr.meter.names == want_names and torch.equal(_bits(tr.meter.table[:len(want_names)]), _bits(want_table))
    _teardown(model, eng)


def _sync_warnings(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return [str(w.message) for w in rec if "synchroniz" in str(w.message).lower()]


def test_diagnostics_add_no_synchronisation(dev):
    """six fit steps under torch.cuda.set_sync_debug_mode('warn'), logging at every step: the run with Diagnostics(level='full') raises
    no more synchronisation warnings than the run without"""
    from valor_amd.train import Trainer
    counts = {}
    for level in (None, "full"):
        _seed_run(77)
        model, eng = _build(dev, 3, _opts(6))
        tr = Trainer(eng, _loaders(), log_fn=lambda *a: None, log_every=1, diagnostics=level)
        counts[level] = _sync_warnings(tr.fit)
        torch.cuda.synchronize()
        assert eng.global_step == 6 and (tr.diagnostics is None) == (level is None)
        _teardown(model, eng)
    print(f"synchronisation warnings: without {len(counts[None])}, with {len(counts['full'])}")
    assert len(counts["full"]) <= len(counts[None]), (counts["full"], counts[None])
