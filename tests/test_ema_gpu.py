"""Weight averaging on the device (valor_amd/ema.py, valor_ema_update): the kernel against its host restatement bit for bit, the average
inside the optimizer and the engine (it does not perturb training, it is the law applied to the masters, a skipped step leaves it), the
in-place swap for evaluation (WeightEMA.applied), exact resume through ckpt/ema_step_N.pt in both save modes, and Trainer.fit validating on
the averaged weights. All comparisons are torch.equal on bit patterns: there is no tolerance in this file.
Engine setup: that of tests/test_train_gpu.py (synth.tiny_spec(), batch 2, 2 frames, 1 audio slice, txt_len 32, bf16)."""
import gc
import os
import random
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TASK_A = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
TASK_B = "pt_contra%tv_mlm%tv"                       # no audio: the audio tower is inactive in every step


@pytest.fixture(autouse=True)
def rng_modes(dev):
    from valor_amd import ops
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    gc.collect()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ the kernel
GUARD = 64                                           # floats on either side of the average: 256 bytes, the buffer stays 16-byte aligned
PATTERN = 0x5A5AC3C3


def _values(n, seed):
    """w, ema of n elements: magnitudes 1e-6 .. 1e3 of both signs; a third of the weights near their average (small differences), some
    equal to it, the rest unrelated; where there is room, pairs whose difference is subnormal"""
    g = torch.Generator().manual_seed(seed)
    mag = lambda: 10.0 ** (torch.rand(n, generator=g) * 9.0 - 6.0) * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)
    e, w = mag(), mag()
    kind = torch.randint(0, 3, (n,), generator=g)
    w = torch.where(kind == 0, e * (1 + 1e-3 * torch.randn(n, generator=g)), w)
    w = torch.where((kind == 1) & (torch.rand(n, generator=g) < 0.2), e, w)
    if n >= 8:
        e[:4] = torch.tensor([1e-38, 3e-41, -2e-39, 1.1754944e-38])
        w[:4] = torch.tensor([1.00001e-38, 1e-41, -2.5e-39, 1.1754942e-38])
        assert bool(((w[:4] - e[:4]).abs() < 1.17549435e-38).all()) and bool(((w[:4] - e[:4]) != 0).all())
    return w.float(), e.float()


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3079, 4099])
def test_kernel_equals_ema_host_bit_for_bit(dev, n):
    """every decay x warm-up x starting count: three updating calls (null gscale, finite, finite) on changing weights, and between the
    second and the third one call with gscale NaN / +inf / -inf that must leave average and count as they are. Around the average a guard
    of a fixed bit pattern, around the count two guard words: a tail overrun would show there."""
    from valor_amd import lib
    from valor_amd.ema import ema_host
    from valor_amd.kernels import _stream
    skips = [float("nan"), float("inf"), float("-inf")]
    combo = 0
    for decay in (0.0, 0.5, 0.9999, 1.0):
        for warmup in (False, True):
            for k0 in (0, 9, 10 ** 6):
                pairs = [_values(n, 1000 * combo + c + n) for c in range(3)]
                ws, e_host = [w for w, _ in pairs], pairs[0][1]
                buf = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=dev).view(torch.float32)
                ema = buf[GUARD:GUARD + n]
                ema.copy_(e_host)
                cbuf = torch.tensor([PATTERN, k0, PATTERN], dtype=torch.int32, device=dev)
                count = cbuf[1:2]
                assert ema.data_ptr() % 16 == 0 and count.data_ptr() % 4 == 0
                fin = torch.tensor(0.37, device=dev)
                bad = torch.tensor(skips[combo % 3], device=dev)
                k = k0

                def call(w_dev, gs):
                    lib.call("valor_ema_update", _stream(), w_dev.data_ptr(), ema.data_ptr(), n, decay, int(warmup), count.data_ptr(),
                             None if gs is None else gs.data_ptr())

                for c, (wi, gs) in enumerate(((0, None), (1, fin), (2, bad), (2, fin))):
                    w = ws[wi]
                    w_dev = w.to(dev)
                    call(w_dev, gs)
                    if gs is not bad:
                        e_host = ema_host(e_host, w, decay, warmup, k)
                        k += 1
                    what = (n, decay, warmup, k0, c)
                    assert _same(ema, e_host), (what, int((_bits(ema) != _bits(e_host)).sum()))
                    assert cbuf.tolist() == [PATTERN, k, PATTERN], (what, cbuf.tolist())
                    assert _same(w_dev, w), what                                               # the weights are read only
                g = buf.view(torch.int32)
                assert bool((g[:GUARD] == PATTERN).all()) and bool((g[GUARD + n:] == PATTERN).all()), (n, decay, warmup, k0)
                assert k == k0 + 3
                combo += 1
    assert combo == 24


def test_kernel_refuses_bad_arguments_on_the_device(dev):
    from valor_amd import lib
    from valor_amd.kernels import _stream
    w, e = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    for args in ((w.data_ptr() + 4, e.data_ptr(), 32, 0.5), (w.data_ptr(), e.data_ptr(), 0, 0.5), (w.data_ptr(), e.data_ptr(), 64, 1.5),
                 (e.data_ptr(), e.data_ptr(), 64, 0.5)):
        with pytest.raises(lib.ValorHipError):
            lib.call("valor_ema_update", _stream(), args[0], args[1], args[2], args[3], 1, cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert float(e.abs().sum()) == 0.0 and int(cnt) == 0


# ------------------------------------------------------------------------------------------------------------------ engine runs
def _opts(steps=100, **kw):
    return SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-4, clip_lr_text=1e-4, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=steps, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0, **kw)


def _build(dev, weight_seed, opts, graphs=True, dtype=torch.bfloat16):
    from valor_amd import synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=weight_seed, w_std=0.05)
    model = VALOR({"dropout": 0.1, "drop_path_rate": 0.0, "token_masker": "host", "seed": 7, "max_generation_len": 8}, spec=spec, dtype=dtype,
                  device=dev)
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


def _batch(dev, i):
    from valor_amd import synth
    b = synth.make_batch(synth.tiny_spec(), batch=2, frames=2, audio_slices=1, txt_len=32, seed=10 + i)
    b["ids"] = [f"clip{i}.{j}" for j in range(2)]
    b["ids_txt"] = list(b["ids"])
    b["video_pixels"], b["audio_spectrograms"] = b["video_pixels"].to(dev), b["audio_spectrograms"].to(dev)
    return b


def _state(eng):
    opt = eng.optimizer
    st = {"flat": eng.model.arena.flat.detach().clone(), "master": opt.master.clone(), "exp_avg": opt.exp_avg.clone(),
          "exp_avg_sq": opt.exp_avg_sq.clone(), "count": opt._count.clone(), "global_step": eng.global_step}
    if eng.ema is not None:
        st["ema"], st["ema_count"] = eng.ema.ema.clone(), eng.ema.count.clone()
    return st


def _same_state(got, want, what, keys=("flat", "master", "exp_avg", "exp_avg_sq", "count")):
    for k in keys:
        assert _same(got[k], want[k]), (what, k, int((_bits(got[k]) != _bits(want[k])).sum()))
    assert got["global_step"] == want["global_step"], what


def _teardown(model, eng):
    from valor_amd import decode
    torch.cuda.synchronize()
    model.enable_graphs(False)
    decode.release_sessions(model)
    eng.close()


_RUNS = {}


def _run(dev, steps, task=TASK_A, dtype=torch.bfloat16, **ema_opts):
    """`steps` engine steps from seed 77 / weights 3, graphs on: the state in front of the first step and behind every step. Computed once
    per configuration and left unchanged."""
    key = (steps, task, dtype, tuple(sorted(ema_opts.items())))
    if key not in _RUNS:
        _seed_run(77)
        model, eng = _build(dev, 3, _opts(**ema_opts), dtype=dtype)
        states = [_state(eng)]
        for s in range(steps):
            eng.train_step(_batch(dev, s), task)
            states.append(_state(eng))
        steps_of, offsets = eng.optimizer.steps, dict(model.arena.offsets)
        _teardown(model, eng)
        _RUNS[key] = (states, SimpleNamespace(steps=steps_of, offsets=offsets))
    return _RUNS[key]


EMA = dict(ema_decay=0.9, ema_warmup=True)


def test_training_is_not_perturbed(dev):
    """5 engine steps with and without an average: parameters, masters, both moments and the per-tensor counts agree to the bit in front
    of the first and behind every step"""
    plain, _ = _run(dev, 5)
    avg, _ = _run(dev, 5, **EMA)
    assert "ema" not in plain[0] and "ema" in avg[0]
    for s in range(6):
        _same_state(avg[s], plain[s], f"step {s}")
    assert not _same(avg[4]["ema"], avg[4]["master"])                        # the average was live


@pytest.mark.parametrize("every", [1, 2])
def test_engine_average_is_the_law(dev, every):
    """the engine's buffer and count after each of 5 steps against ema_host replayed on clones of the masters; then, at optimizer level, a
    step whose gradient arena holds an inf (average and count stay) and a finite one (the law continues)"""
    from valor_amd.ema import ema_host
    opts = dict(EMA) if every == 1 else dict(EMA, ema_every=every)
    states, _ = _run(dev, 5, **opts)
    assert _same(states[0]["ema"], states[0]["master"]) and int(states[0]["ema_count"]) == 0        # seeded from the fp32 masters
    e, k = states[0]["master"].cpu(), 0
    for s in range(1, 6):
        if s % every == 0:
            e = ema_host(e, states[s]["master"].cpu(), 0.9, True, k)
            k += 1
        assert _same(states[s]["ema"], e), (s, int((_bits(states[s]["ema"]) != _bits(e)).sum()))
        assert int(states[s]["ema_count"]) == k, (s, k)
    assert k == 5 // every
    if every != 1:
        return
    # optimizer level: the same run again, then an inf written into the gradient arena by the test
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(**opts))
    for s in range(5):
        eng.train_step(_batch(dev, s), TASK_A)
    opt, ema, a = eng.optimizer, eng.ema, model.arena
    assert _same(ema.ema, e) and ema.updates == 5
    before_master = opt.master.clone()
    a.grad.copy_((torch.randn(a.numel, device=dev) * 1e-3).to(a.dtype))
    o, cnt, _ = a.offsets[list(a.offsets)[len(a.offsets) // 2]]
    a.grad[o + cnt // 2] = float("inf")
    opt.step(max_grad_norm=5.0, ema=ema)
    assert not torch.isfinite(opt.total_norm)
    assert _same(ema.ema, e) and ema.updates == 5 and _same(opt.master, before_master)
    a.grad.copy_((torch.randn(a.numel, device=dev) * 1e-3).to(a.dtype))
    opt.step(max_grad_norm=5.0, ema=ema)
    assert not _same(opt.master, before_master)
    e = ema_host(e, opt.master.cpu(), 0.9, True, 5)
    assert _same(ema.ema, e) and ema.updates == 6
    _teardown(model, eng)


def test_inactive_tensors_equal_their_average(dev):
    """a task without audio: the audio tower receives no gradient in any step, its masters never move, and its average equals them to
    the bit although the kernel runs over the whole arena; the active tensors' averages trail their masters"""
    states, info = _run(dev, 3, task=TASK_B, **EMA)
    idle = [n for n, c in info.steps.items() if c == 0]
    busy = [n for n, c in info.steps.items() if c == 3]
    assert idle and busy and any("audio" in n for n in idle)
    ema, master = states[3]["ema"], states[3]["master"]
    cut = lambda t, n: t[info.offsets[n][0]:info.offsets[n][0] + info.offsets[n][1]]
    for n in idle:
        assert _same(cut(ema, n), cut(master, n)), n
    assert any(not _same(cut(ema, n), cut(master, n)) for n in busy)
    assert int(states[3]["ema_count"]) == 3


# ------------------------------------------------------------------------------------------------------------------ applied()
def _eval_outputs(model, dev):
    """an evaluation-mode forward with losses (the host masker's draws pinned), one without (features and scores), and the greedy
    captions of one batch"""
    from valor_amd import decode
    model.eval()
    batch = _batch(dev, 40)
    out = {}
    with torch.no_grad():
        random.seed(5)
        for k, v in model(batch, task=TASK_A, compute_loss=True).items():
            out["loss/" + k] = v.detach().clone()
        random.seed(5)
        for k, v in model(batch, task=TASK_A, compute_loss=False).items():
            if isinstance(v, torch.Tensor):
                out["eval/" + k] = v.detach().clone()
    for k, v in decode.generate_cap(model, batch, ["tv"], mode="greedy").items():
        if isinstance(v, torch.Tensor):
            out["gen/" + k] = v.detach().clone()
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_applied_swaps_in_place_and_restores(dev, dtype, tmp_path):
    """graphs on (the default). 4 steps, a generation on the training weights (it leaves a decoding session behind), then applied():
    the arena is the cast average, evaluation and greedy generation equal those of a fresh model that loaded state_dict()['weights'];
    after exit arena and masters are what they were and step 5 equals that of a run that never entered applied()."""
    from valor_amd import checkpoint, decode
    from valor_amd.model.valor import VALOR
    from valor_amd import synth
    opts = dict(ema_decay=0.5, ema_warmup=False)
    want, _ = _run(dev, 5, dtype=dtype, **opts)
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(**opts), dtype=dtype)
    for s in range(4):
        eng.train_step(_batch(dev, s), TASK_A)
    _same_state(_state(eng), want[4], "step 4", keys=("flat", "master", "ema", "ema_count"))
    ema, arena = eng.ema, model.arena
    host_rng = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    decode.generate_cap(model, _batch(dev, 40), ["tv"], mode="greedy")             # a session with the training weights' K|V stays behind
    live, master, addr = arena.flat.clone(), eng.optimizer.master.clone(), arena.flat.data_ptr()
    sd = ema.state_dict()
    fresh = VALOR({"dropout": 0.1, "drop_path_rate": 0.0, "token_masker": "host", "seed": 7, "max_generation_len": 8}, spec=synth.tiny_spec(),
                  dtype=dtype, device=dev)
    fresh.load_state_dict(sd["weights"], strict=True)
    ref = _eval_outputs(fresh, dev)
    decode.release_sessions(fresh)
    assert any(k.startswith("loss/") for k in ref) and any(k.startswith("eval/feat") for k in ref) and any(k.startswith("gen/") for k in ref)
    with ema.applied():
        assert arena.flat.data_ptr() == addr and _same(arena.flat, ema.ema.to(dtype)) and not _same(arena.flat, live)
        assert _same(arena.flat, fresh.arena.flat)
        got = _eval_outputs(model, dev)
        assert got.keys() == ref.keys()
        for k in ref:
            assert _same(got[k], ref[k]), k
        with pytest.raises(RuntimeError, match="re-entrant"):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError, match="applied"):
            eng.train_step(_batch(dev, 4), TASK_A)
        with pytest.raises(RuntimeError, match="applied"):
            checkpoint.save_run(eng, str(tmp_path))
        assert _same(arena.flat, fresh.arena.flat)                                 # none of the refusals restored or wrote anything
        if dtype != torch.float32:
            assert _same(eng.optimizer.master, master)                             # (fp32 parity mode: the parameters are the masters)
    assert not os.path.isdir(tmp_path / "ckpt") or os.listdir(tmp_path / "ckpt") == []
    assert _same(arena.flat, live) and _same(eng.optimizer.master, master) and eng.global_step == 4

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with ema.applied():
            assert not _same(arena.flat, live)
            raise Boom()
    assert _same(arena.flat, live) and _same(eng.optimizer.master, master)
    decode.release_sessions(model)
    random.setstate(host_rng[0]); np.random.set_state(host_rng[1]); torch.set_rng_state(host_rng[2])
    eng.train_step(_batch(dev, 4), TASK_A)
    _same_state(_state(eng), want[5], "step 5 behind applied()", keys=("flat", "master", "exp_avg", "exp_avg_sq", "count", "ema", "ema_count"))
    _teardown(model, eng)


# ------------------------------------------------------------------------------------------------------------------ resume
@pytest.mark.parametrize("blocking", [True, False], ids=["blocking", "nonblocking"])
def test_resume_continues_the_average_to_the_bit(dev, tmp_path, blocking):
    from valor_amd import checkpoint
    want, _ = _run(dev, 4, **EMA)
    run = str(tmp_path)
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(**EMA))
    for s in range(2):
        eng.train_step(_batch(dev, s), TASK_A)
    h = checkpoint.save_run(eng, run, blocking=blocking)
    eng.train_step(_batch(dev, 2), TASK_A)                     # the run goes on while a non-blocking save is written: the file holds step 2
    h.wait()
    _teardown(model, eng)
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["ema_step_2.pt", "engine_step_2.rank0.pt", "model_step_2.pt", "optimizer_step_2.pt"]
    sd = torch.load(checkpoint.ema_file(run, 2), map_location="cpu", weights_only=True)
    assert sd["count"] == 2 and sd["decay"] == 0.9 and sd["warmup"] is True and sd["every"] == 1

    _seed_run(4000)                                             # a process state in which only the load can make the runs agree
    model, eng = _build(dev, 11, _opts(**EMA))
    assert not _same(eng.ema.ema, want[2]["ema"])
    assert checkpoint.resume_run(eng, run) == 2
    _same_state(_state(eng), want[2], "loaded", keys=("flat", "master", "exp_avg", "exp_avg_sq", "count", "ema", "ema_count"))
    for s in (2, 3):
        eng.train_step(_batch(dev, s), TASK_A)
    _same_state(_state(eng), want[4], "resumed, step 4", keys=("flat", "master", "exp_avg", "exp_avg_sq", "count", "ema", "ema_count"))
    checkpoint.save_run(eng, run, blocking=blocking).wait()    # remove_before_ckpt (the default): the older average goes with its step
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["ema_step_4.pt", "engine_step_4.rank0.pt", "model_step_4.pt", "optimizer_step_4.pt"]
    _teardown(model, eng)
    if not blocking:
        return
    # an engine without an average resumes from a directory that has the file
    _seed_run(4000)
    model, eng = _build(dev, 11, _opts())
    assert eng.ema is None and checkpoint.resume_run(eng, run) == 4
    _same_state(_state(eng), want[4], "no average")
    _teardown(model, eng)
    # without the file
    os.remove(checkpoint.ema_file(run, 4))
    _seed_run(4000)
    model, eng = _build(dev, 11, _opts(**EMA))
    before = model.arena.flat.clone()
    with pytest.raises(FileNotFoundError, match="ema_step_4.pt"):
        checkpoint.resume_run(eng, run)
    assert _same(model.arena.flat, before) and eng.global_step == 0
    assert checkpoint.resume_run(eng, run, allow_inexact=True) == 4
    assert _same(eng.optimizer.master, want[4]["master"]) and _same(eng.ema.ema, want[4]["master"]) and eng.ema.updates == 0
    _teardown(model, eng)


# ------------------------------------------------------------------------------------------------------------------ Trainer.fit
class SynthLoader:
    def __init__(self, n, seed0):
        self.n, self.seed0 = n, seed0

    def __iter__(self):
        from valor_amd import synth
        for i in range(self.n):
            b = synth.make_batch(synth.tiny_spec(), batch=2, frames=2, audio_slices=1, txt_len=32, seed=self.seed0 + i)
            b["ids"] = [f"t{i}.{j}" for j in range(2)]
            yield b


def _loaders():
    from valor_amd.train import MetaLoader
    return MetaLoader({TASK_A + "--dsetA": SynthLoader(3, 10), TASK_B + "--dsetB": SynthLoader(2, 500)}, seed=4)


def test_fit_validates_on_the_averaged_weights(dev, tmp_path):
    """4 steps, a ret%tv validation of 4 clips behind the steps 1 and 3, ema_eval='both': the metrics of step 3 are those of
    evaluate.validate under applied() on the checkpoint of that step, the live/ entries those of a validation outside it, the best-metric
    history follows the averaged weights, and the checkpoint folder holds the average"""
    from valor_amd import checkpoint, evaluate, synth
    from valor_amd.train import Trainer
    spec = synth.tiny_spec()
    vb = []
    for i in range(2):
        b = synth.make_batch(spec, batch=2, frames=2, audio_slices=1, txt_len=32, seed=900 + i)
        b["ids"] = [f"v{2 * i + j}" for j in range(2)]
        b["ids_txt"] = list(b["ids"])
        vb.append(b)
    val = {"ret%tv--dsetV": vb}
    ema_opts = dict(ema_decay=0.5, ema_warmup=False, ema_eval="both")
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(4, valid_steps=2, **ema_opts))
    logged = []
    out = Trainer(eng, _loaders(), val_loaders=val, output_dir=str(tmp_path), log_fn=lambda s, sc: logged.append((s, sc))).fit()
    assert out["global_step"] == 4 and sorted(out["validations"]) == [1, 3] and out["checkpoints"] == [1, 3]
    assert model.training and "_decode_sessions" not in model.__dict__ and eng.ema.updates == 4
    names = sorted(os.listdir(tmp_path / "ckpt"))
    assert names == ["ema_step_3.pt", "engine_step_3.rank0.pt", "model_step_3.pt", "optimizer_step_3.pt", "train_step_3.rank0.pt"], names
    assert set(out["validations"][3]) == {"ret%tv--dsetV", "live/ret%tv--dsetV"}
    live_logged = [sc for s, sc in logged if s == 3 and any(k.startswith("live/") for k in sc)]
    assert live_logged and live_logged[0]["live/ret%tv--dsetV_t_v"] == out["validations"][3]["live/ret%tv--dsetV"]["t_v"]
    _teardown(model, eng)
    # by hand on the checkpoint of step 3
    _seed_run(5)
    model2, eng2 = _build(dev, 11, _opts(4, valid_steps=2, **ema_opts))
    assert checkpoint.resume_run(eng2, str(tmp_path)) == 3 and eng2.ema.updates == 3
    with eng2.ema.applied():
        averaged = evaluate.validate(model2, val)
    live = evaluate.validate(model2, val)
    assert averaged["ret%tv--dsetV"] == out["validations"][3]["ret%tv--dsetV"]
    assert live["ret%tv--dsetV"] == out["validations"][3]["live/ret%tv--dsetV"]
    hist = out["best"]["ret%tv--dsetV_t_v"]
    assert hist["3"] == averaged["ret%tv--dsetV"]["t_v"] and set(hist) == {"1", "3", "best_step", "best_value"}
    assert hist["best_value"] == max(hist["1"]["video_ravg"], hist["3"]["video_ravg"])
    _teardown(model2, eng2)


def _sync_warnings(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return [str(w.message) for w in rec if "synchroniz" in str(w.message).lower()]


def test_the_average_adds_no_synchronisation(dev):
    """6 fit steps (no validation, no log snapshots) under torch.cuda.set_sync_debug_mode('warn'): as many synchronisation warnings with
    ema_decay set as without"""
    from valor_amd.train import Trainer
    probe = torch.ones((), device=dev)
    if not _sync_warnings(lambda: probe.item()):
        pytest.skip("torch.cuda.set_sync_debug_mode('warn') is not live in this build: a deliberate .item() did not warn")
    counts = {}
    for tag, extra in (("plain", {}), ("ema", dict(ema_decay=0.9999, ema_every=2))):
        _seed_run(77)
        model, eng = _build(dev, 3, _opts(6, **extra))
        tr = Trainer(eng, _loaders(), log_fn=lambda *a: None, log_every=10 ** 6)
        counts[tag] = _sync_warnings(tr.fit)
        torch.cuda.synchronize()
        assert eng.global_step == 6 and (eng.ema is None) == (tag == "plain")
        if eng.ema is not None:
            assert eng.ema.updates == 3
        _teardown(model, eng)
    print(f"synchronisation warnings: plain {len(counts['plain'])}, with the average {len(counts['ema'])}")
    assert len(counts["ema"]) == len(counts["plain"]), (len(counts["ema"]), len(counts["plain"]))
