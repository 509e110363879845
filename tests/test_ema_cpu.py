"""CPU: the host side of weight averaging (valor_amd/ema.py): the law's restatement ema_host against fp64, the warm-up schedule, the
argument checks of valor_ema_update (no launch is reached), and the file logic on CPU-built models as tests/test_resume_cpu.py does it:
ckpt/ema_step_N.pt beside the run's files, invisible to the reference's listings, state_dict / load_state_dict to the bit, resume with and
without the file. The kernel itself, bit for bit against ema_host, is tests/test_ema_gpu.py."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from valor_amd import checkpoint, ops, synth
from valor_amd.ema import WeightEMA, decay_at, ema_host
from valor_amd.engine import TrainEngine
from valor_amd.model.valor import VALOR

U = 2.0 ** -24                 # unit roundoff of fp32
DECAYS = [0.0, 0.5, 0.9999, 1.0]


@pytest.fixture(autouse=True)
def host_mode():
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", DECAYS)
def test_ema_host_against_fp64(decay, warmup):
    """300 steps of ema_host on 4096 elements against the same recurrence E <- E + a (w - E) in fp64, with the SAME fp32 a = fl(1 - d) per
    step (the schedule is checked on its own below), the weights a random walk of scale 1.

    The bound. One fp32 step computes t^ = (w - e)(1 + e1), p^ = a t^ (1 + e2), e' = (e + p^)(1 + e3) with |ei| <= u = 2^-24 (a
    subnormal product adds at most 2^-150; sums and differences are exact there). Against the exact step from the same e the result
    is off by r with |r| <= a |w - e| (2u + u^2) + |e + p^| u. With M >= |w|, |e| (the average stays inside the hull of its inputs up to
    rounding; M carries 1e-3 of slack for that): |w - e| <= 2M and |e + p^| <= M, so |r| <= u M (4a (1 + u) + 1). An error delta already
    in e is carried through the exact step as (1 - a) delta -- the contraction by d. Hence B' = (1 - a) B + u M (4a (1 + u) + 1) + 2^-149,
    B0 = 0, evaluated step by step in fp64 with the step's own a: about u M (1 + 4a) / a once it has settled, u M n for a = 0."""
    g = torch.Generator().manual_seed(5)
    n, steps = 4096, 300
    w = torch.randn(n, generator=g)
    e32 = torch.randn(n, generator=g)
    e64 = e32.double()
    walk = [w]
    for _ in range(steps - 1):
        walk.append(walk[-1] + 0.05 * torch.randn(n, generator=g))
    M = max(float(e32.abs().max()), max(float(x.abs().max()) for x in walk)) * 1.001
    bound, worst = 0.0, 0.0
    for k, wk in enumerate(walk):
        a = float(np.float32(1) - decay_at(decay, warmup, k))
        e32 = ema_host(e32, wk, decay, warmup, k)
        e64 = e64 + a * (wk.double() - e64)
        bound = (1.0 - a) * bound + U * M * (4.0 * a * (1.0 + U) + 1.0) + 2.0 ** -149
        err = float((e32.double() - e64).abs().max())
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
    assert e32.dtype == torch.float32
    print(f"decay {decay} warmup {warmup}: final error {err:.3e}, bound {bound:.3e}, worst ratio {worst:.3f}")


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
def test_decay_one_never_moves_and_equal_stays_equal(warmup):
    g = torch.Generator().manual_seed(6)
    e0 = torch.randn(2048, generator=g) * 100.0
    e = e0.clone()
    # decay = 1 without warm-up: a = 0, the product is +-0 and e + 0 = e. (With warm-up d = (1 + k) / (10 + k) < 1 until it is clamped.)
    for k in range(20):
        e = ema_host(e, torch.randn(2048, generator=g), 1.0, False, k)
    assert torch.equal(_bits(e), _bits(e0))
    # w == ema: t = 0 exactly, whatever d
    vals = torch.cat([e0, torch.tensor([0.0, 1e-45, -1e-45, 1e-38, 3.4e38, -3.4e38, 1e-6, 1e3])])
    for decay in DECAYS + [0.3]:
        for k in (0, 1, 9, 10 ** 6):
            out = ema_host(vals.clone(), vals.clone(), decay, warmup, k)
            assert torch.equal(_bits(out), _bits(vals)), (decay, k)


def test_decay_zero_copies_the_weights():
    """decay = 0: a = 1, ema' = fl(ema + fl(w - ema)). On data whose difference is exact -- both on the grid 2^-10 Z below 2^10, so the
    difference is a multiple of 2^-10 below 2^11: 21 bits -- the sum is w itself. Otherwise fl(w - ema) = (w - ema)(1 + e1) and the sum
    rounds once more: |ema' - w| <= (u |w - ema| + u |w|)(1 + u), per element."""
    g = torch.Generator().manual_seed(7)
    grid = lambda: torch.randint(-2 ** 20 + 1, 2 ** 20, (4096,), generator=g).float() / 1024.0
    w, e = grid(), grid()
    assert torch.equal((w.double() - e.double()).float().double(), w.double() - e.double())          # the construction holds
    assert torch.equal(_bits(ema_host(e, w, 0.0, False, 0)), _bits(w))
    assert torch.equal(_bits(ema_host(e, w, 0.0, False, 10 ** 6)), _bits(w))
    w = torch.randn(4096, generator=g) * 1e-3              # small weights under a large average: w - ema drops w's low bits
    e = torch.randn(4096, generator=g) * 1e3
    out = ema_host(e, w, 0.0, False, 0)
    lim = (U * (w.double() - e.double()).abs() + U * w.double().abs()) * (1 + U)
    assert bool(((out.double() - w.double()).abs() <= lim).all())
    assert not torch.equal(out, w)                                                              # the rounding case was live


def test_warmup_schedule_values():
    f = np.float32
    assert decay_at(0.9999, True, 0) == f(1) / f(10) == f(0.1)
    assert decay_at(0.9999, True, 1) == f(2) / f(11)
    assert decay_at(0.9999, True, 9) == f(10) / f(19)
    assert decay_at(0.9999, True, 10 ** 6) == f(0.9999)                      # (10^6 + 1) / (10^6 + 10) = 0.999991 > 0.9999: clamped
    assert decay_at(1.0, True, 10 ** 6) == f(1000001) / f(1000010) == f(1000001 / 1000010)
    assert decay_at(0.05, True, 0) == f(0.05)                                # a small decay is never raised
    for k in (0, 1, 9, 10 ** 6):
        assert decay_at(0.9999, False, k) == f(0.9999)
        assert decay_at(0.9999, True, k).dtype == np.float32
    # both integers convert exactly and the quotient is one correctly rounded division: it equals the fp64 quotient rounded once
    for k in (0, 1, 9, 12345, 10 ** 6):
        assert decay_at(1.0, True, k) == f((1 + k) / (10 + k))


# ------------------------------------------------------------------------------------------------------------------ the entry point
def test_ema_update_argument_validation_without_gpu():
    """every VALOR_ERR_ARG case of valor_ema_update is decided before any launch. Each call differs from a valid one in one argument."""
    from valor_amd import lib
    so = lib.load()
    w, e = torch.zeros(64), torch.zeros(64)
    cnt = torch.zeros(4, dtype=torch.int32)
    gs = torch.ones(4)
    pw, pe, pc, pg = w.data_ptr(), e.data_ptr(), cnt.data_ptr(), gs.data_ptr()
    assert pw % 16 == 0 and pe % 16 == 0 and pc % 4 == 0
    call = lambda w_=pw, e_=pe, n=64, decay=0.5, warmup=1, c=pc, g=pg: so.valor_ema_update(None, w_, e_, n, decay, warmup, c, g)
    assert call(w_=None) == -1 and call(e_=None) == -1 and call(c=None) == -1          # null pointers (a null gscale is allowed)
    assert call(n=0) == -1 and call(n=-4) == -1
    for bad in (-1e-6, 1.0 + 1e-6, 2.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(decay=bad) == -1, bad
    assert call(w_=pw + 4, n=32) == -1 and call(e_=pe + 8, n=32) == -1                   # not 16-byte aligned
    assert call(c=pc + 2) == -1 and call(g=pg + 1) == -1                                # not 4-byte aligned
    assert call(w_=pe) == -1 and call(w_=pe + 16, n=32) == -1 and call(w_=pe, e_=pe + 16, n=32) == -1      # overlapping buffers
    assert (w == 0).all() and (e == 0).all() and (cnt == 0).all()
    prev = so.valor_ema_set_nt(-1)
    assert prev in (0, 1, 2, 3) and so.valor_ema_set_nt(-1) == prev                     # a query changes nothing


def test_constructor_refuses_bad_settings():
    model, eng = _engine()
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            WeightEMA(eng.optimizer, bad)
    with pytest.raises(ValueError, match="every"):
        WeightEMA(eng.optimizer, 0.5, every=0)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ files
def _engine(dtype=torch.bfloat16, weight_seed=3, **opts):
    spec = synth.tiny_spec()
    model = VALOR({"dropout": 0.1, "token_masker": "host"}, spec=spec, dtype=dtype, device="cpu")
    model.load_state_dict(synth.make_state_dict(spec, seed=weight_seed))
    o = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, betas=[0.9, 0.98], num_train_steps=100, warmup_ratio=0.1, **opts)
    return model, TrainEngine(model, o, manage_gc=False)


def _stir(ema, seed, count):
    """an average that differs from the masters everywhere, and a count"""
    ema.ema.add_(torch.randn(ema.ema.numel(), generator=torch.Generator().manual_seed(seed)) * 1e-3)
    pad = torch.ones(ema.ema.numel(), dtype=torch.bool)                  # pads stay zero, as the kernel keeps them
    for o, n, _ in ema.arena.offsets.values():
        pad[o:o + n] = False
    ema.ema[pad] = 0.0
    ema.count.fill_(count)
    ema._started = True


def test_options_build_the_average_and_off_is_off():
    model, eng = _engine()
    assert eng.ema is None and not hasattr(eng.optimizer, "_emas")
    eng.close()
    model, eng = _engine(ema_decay=0.999, ema_warmup=False, ema_every=3)
    e = eng.ema
    assert isinstance(e, WeightEMA) and (e.decay, e.warmup, e.every) == (0.999, False, 3)
    assert e.ema.dtype == torch.float32 and e.ema.numel() == model.arena.numel and torch.equal(e.ema, eng.optimizer.master)
    assert e.ema.data_ptr() != eng.optimizer.master.data_ptr() and e.updates == 0
    # masters rewritten before the first update (weights loaded after the optimizer exists): the average follows
    sd = synth.make_state_dict(synth.tiny_spec(), seed=9)
    model.load_state_dict(sd)
    eng.optimizer.init_master_from(sd)
    assert torch.equal(e.ema, eng.optimizer.master)
    # ... and not once it has started
    _stir(e, 1, 5)
    kept = e.ema.clone()
    model.load_state_dict(synth.make_state_dict(synth.tiny_spec(), seed=10))
    assert torch.equal(e.ema, kept) and e.updates == 5
    eng.close()


def test_state_dict_round_trip_to_the_bit(tmp_path):
    model, eng = _engine(ema_decay=0.9999)
    _stir(eng.ema, 2, 1234)
    sd = eng.ema.state_dict()
    assert sd["count"] == 1234 and sd["decay"] == 0.9999 and sd["warmup"] is True and sd["every"] == 1
    assert all(v.dtype == torch.float32 for v in sd["weights"].values() if v.is_floating_point())
    assert set(sd["weights"]) == set(model.state_dict())                                    # the model's keys, the reference's layout
    # the weights entry is a model checkpoint: a model that loads it holds the rounded average
    model_b = VALOR({"dropout": 0.1}, spec=synth.tiny_spec(), dtype=torch.bfloat16, device="cpu")
    model_b.load_state_dict(sd["weights"], strict=True)
    assert torch.equal(model_b.arena.flat, eng.ema.ema.to(torch.bfloat16))
    path = tmp_path / "e.pt"
    torch.save(checkpoint._host_copy(sd), path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    model2, eng2 = _engine(weight_seed=4, ema_decay=0.5, ema_warmup=False, ema_every=7)
    assert not torch.equal(eng2.ema.ema, eng.ema.ema)
    eng2.ema.load_state_dict(back)
    assert torch.equal(_bits(eng2.ema.ema), _bits(eng.ema.ema)) and eng2.ema.updates == 1234
    assert (eng2.ema.decay, eng2.ema.warmup, eng2.ema.every) == (0.9999, True, 1)
    with pytest.raises(ValueError, match="format"):
        eng2.ema.load_state_dict(dict(back, format="something/0"))
    drop = next(iter(eng.optimizer._ref_slices()))
    short = dict(back, weights={k: v for k, v in back["weights"].items() if k != drop})
    with pytest.raises(RuntimeError, match="missing"):
        eng2.ema.load_state_dict(short)
    eng.close(); eng2.close()


def test_ema_file_is_invisible_to_the_reference_listings(tmp_path):
    """train_utils.py:174-187 and inference.py:65-66 list the checkpoint folder with startswith('model') / startswith('optimizer') and
    parse the step out of every such name"""
    model, eng = _engine(ema_decay=0.999)
    eng.global_step = 6
    h = checkpoint.save_run(eng, str(tmp_path))
    names = sorted(os.listdir(tmp_path / "ckpt"))
    assert names == ["ema_step_6.pt", "engine_step_6.rank0.pt", "model_step_6.pt", "optimizer_step_6.pt"]
    assert h.files["ema"] == checkpoint.ema_file(str(tmp_path), 6)
    models = [n for n in names if n.startswith("model")]
    optims = [n for n in names if n.startswith("optimizer")]
    assert models == ["model_step_6.pt"] and optims == ["optimizer_step_6.pt"]
    assert [int(n.split(".")[0].split("_")[-1]) for n in models] == [6]                      # the reference's parse
    assert checkpoint.latest_step(str(tmp_path)) == 6
    (tmp_path / "ckpt" / "ema_step_50.pt").write_bytes(b"")                                   # an average alone is no checkpoint
    assert checkpoint.latest_step(str(tmp_path)) == 6
    assert set(checkpoint.run_files(str(tmp_path), 6)) == {"model", "optimizer", "engine"}
    eng.close()


def test_save_resume_and_removal_on_the_host(tmp_path):
    model, eng = _engine(ema_decay=0.999)
    _stir(eng.ema, 3, 2)
    eng.global_step = 2
    checkpoint.save_run(eng, str(tmp_path))
    _stir(eng.ema, 4, 4)
    eng.global_step = 4
    checkpoint.save_run(eng, str(tmp_path))
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["ema_step_4.pt", "engine_step_4.rank0.pt", "model_step_4.pt", "optimizer_step_4.pt"]
    model2, eng2 = _engine(weight_seed=4, ema_decay=0.999)
    assert checkpoint.resume_run(eng2, str(tmp_path)) == 4
    assert torch.equal(_bits(eng2.ema.ema), _bits(eng.ema.ema)) and eng2.ema.updates == 4
    assert torch.equal(eng2.optimizer.master, eng.optimizer.master)
    # an engine without an average ignores the file
    model3, eng3 = _engine(weight_seed=5)
    assert checkpoint.resume_run(eng3, str(tmp_path)) == 4 and eng3.ema is None
    assert torch.equal(model3.arena.flat, model.arena.flat)
    # without the file: refused before anything is loaded, then explicit
    os.remove(checkpoint.ema_file(str(tmp_path), 4))
    model4, eng4 = _engine(weight_seed=6, ema_decay=0.999)
    before = model4.arena.flat.clone()
    with pytest.raises(FileNotFoundError, match="ema_step_4.pt"):
        checkpoint.resume_run(eng4, str(tmp_path))
    assert torch.equal(model4.arena.flat, before) and eng4.global_step == 0
    assert checkpoint.resume_run(eng4, str(tmp_path), allow_inexact=True) == 4
    assert torch.equal(eng4.ema.ema, eng4.optimizer.master) and torch.equal(eng4.optimizer.master, eng.optimizer.master)
    assert eng4.ema.updates == 0
    # a run without an average writes what it wrote before
    eng3.global_step = 5
    checkpoint.save_run(eng3, str(tmp_path))
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["engine_step_5.rank0.pt", "model_step_5.pt", "optimizer_step_5.pt"]
    for e in (eng, eng2, eng3, eng4):
        e.close()


def test_applied_on_the_host_in_parity_mode(tmp_path):
    """fp32 parity mode needs no kernel for the swap (the cast is a copy): the protocol of applied() without a device"""
    model, eng = _engine(dtype=torch.float32, ema_decay=0.999)
    ema = eng.ema
    _stir(ema, 8, 3)
    live = model.arena.flat.clone()
    addr = model.arena.flat.data_ptr()
    with ema.applied() as got:
        assert got is ema and torch.equal(model.arena.flat, ema.ema) and not torch.equal(model.arena.flat, live)
        assert model.arena.flat.data_ptr() == addr and model.P["contra_temp"].data_ptr() == addr + 4 * model.arena.offsets["contra_temp"][0]
        with pytest.raises(RuntimeError, match="re-entrant"):
            with ema.applied():
                pass
        assert torch.equal(model.arena.flat, ema.ema)                        # the refused entry restored nothing
        with pytest.raises(RuntimeError, match="applied"):
            eng.train_step({}, "pt_mlm%tva")
        with pytest.raises(RuntimeError, match="applied"):
            eng.train_window([{}], "pt_contra%tv")
        with pytest.raises(RuntimeError, match="applied"):
            checkpoint.save_run(eng, str(tmp_path))
    assert torch.equal(_bits(model.arena.flat), _bits(live)) and eng.global_step == 0
    assert not os.path.isdir(tmp_path / "ckpt") or os.listdir(tmp_path / "ckpt") == []

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with ema.applied():
            raise Boom()
    assert torch.equal(_bits(model.arena.flat), _bits(live))
    with ema.applied():                                                      # and it can be entered again
        pass
    assert torch.equal(_bits(model.arena.flat), _bits(live))
    eng.close()
