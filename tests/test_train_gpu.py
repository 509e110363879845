"""The training driver on the device (valor_amd/train.py): the loss meter's kernel against its numpy restatement, Trainer.fit against the
hand-written loop of train_step calls, exact resume through the driver (loader position and meter included), validation inside the loop,
and the count of host synchronisations. Setup is that of tests/test_resume_gpu.py: synth.tiny_spec(), batch 2, 2 frames, 1 audio slice,
txt_len 32, bf16. All comparisons are torch.equal / ==: no tolerance anywhere."""
import gc
import os
import random
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
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


# ------------------------------------------------------------------------------------------------------------------ the meter
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_meter_matches_meter_host_bit_for_bit(dev):
    """300 updates of n = 1, 5 and 32 sources into 40 rows, values from a seeded generator with NaN, +inf and -inf planted, the row subset
    changing between calls; after a state_dict round trip the next 50 updates still agree. This test fails without the feature."""
    from valor_amd.lib import METER_FIELDS
    from valor_amd.train import LossMeter, meter_host
    rng = np.random.default_rng(11)
    total, width = 350, 32
    vals = (rng.standard_normal((total, width)) * rng.choice([1e-3, 1.0, 300.0], size=(total, width))).astype(np.float32)
    plant = rng.random((total, width))
    vals[plant < 0.05] = np.nan
    vals[(plant >= 0.05) & (plant < 0.07)] = np.inf
    vals[(plant >= 0.07) & (plant < 0.09)] = -np.inf
    vals[0, 0] = np.nan                                    # a key whose first value is not finite: the first finite one starts its average
    dvals = torch.from_numpy(vals).to(dev)
    keys = [f"k{j}" for j in range(40)]
    meter = LossMeter(dev, rows=8)                         # 8 rows: the table grows twice on the way to 40
    seen = {k: [] for k in keys}

    def run(m, first, count):
        for i in range(first, first + count):
            n = (1, 5, 32)[i % 3]
            pick = [keys[j] for j in rng.choice(40, size=n, replace=False)]
            if i % 2:
                m.update("task--dset", {k: dvals[i, c] for c, k in enumerate(pick)})
            else:                                          # the same through `extra`, whose keys are taken as they are
                m.update("task--dset", {}, {f"loss_task--dset/{k}": dvals[i, c] for c, k in enumerate(pick)})
            for c, k in enumerate(pick):
                seen[k].append(vals[i, c])

    def check(m, what):
        assert set(m.names) == {f"loss_task--dset/{k}" for k in keys if seen[k]}, what
        table = m.table.cpu()
        for k in keys:
            if not seen[k]:
                continue
            want = meter_host(seen[k], m.keep, m.take)
            got = table[m.rows[f"loss_task--dset/{k}"]]
            assert torch.equal(_bits(got), _bits(torch.from_numpy(want))), (what, k, got.tolist(), want.tolist())
        assert torch.equal(_bits(table[len(m.names):]), _bits(m._fresh(table.shape[0])[len(m.names):])), what      # untouched rows

    run(meter, 0, 300)
    assert len(meter.names) == 40 and meter.table.shape[0] >= 40
    check(meter, "300 updates")
    assert any(np.isnan(meter_host(seen[k], meter.keep, meter.take)[0]) for k in keys)           # the planted values were live
    assert sum(int(meter_host(seen[k], meter.keep, meter.take)[6]) for k in keys) > 100
    # snapshot / poll / flush: what comes back is the table
    meter.snapshot(step=300, host={"lr_ratio": 0.5})
    got = meter.flush(step=301)
    assert [s for s, _ in got] == [300, 301] and got[0][1]["lr_ratio"] == 0.5 and meter.poll() == []
    table = meter.table.cpu()
    for k in keys:
        row, rec = table[meter.rows[f"loss_task--dset/{k}"]].tolist(), got[1][1][f"loss_task--dset/{k}"]
        assert list(rec) == list(METER_FIELDS[:7])
        assert all(a == b or (a != a and b != b) for a, b in zip(rec.values(), row))
    # the round trip: a fresh meter continues every average to the bit
    sd = meter.state_dict()
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"valor_meter_state_{os.getpid()}.pt")
    torch.save(sd, path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    os.remove(path)
    fresh = LossMeter(dev, rows=8)
    fresh.load_state_dict(sd)
    assert fresh.names == meter.names and torch.equal(_bits(fresh.table[:40]), _bits(meter.table[:40]))
    run(fresh, 300, 50)
    check(fresh, "50 updates behind the round trip")
    assert not torch.equal(_bits(fresh.table[:40]), _bits(meter.table[:40]))


def test_meter_kernel_refuses_bad_arguments_on_the_device(dev):
    from valor_amd import kernels, lib
    table = torch.zeros((4, 8), device=dev)
    x = torch.ones((), device=dev)
    with pytest.raises(lib.ValorHipError):
        kernels.meter_update(table, [x, x.clone()], [1, 1], 0.99, 0.01)
    with pytest.raises(lib.ValorHipError):
        kernels.meter_update(table, [x], [4], 0.99, 0.01)
    torch.cuda.synchronize()
    assert float(table.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ the driver
class Sampler:
    def __init__(self):
        self.epoch = 0

    def set_epoch(self, e):
        self.epoch = e


class SynthLoader:
    """`n` batches per epoch; batch i of epoch e is synth.make_batch(seed = seed0 + 100 e + i): a function of (epoch, index)"""

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


def _build(dev, weight_seed, opts, graphs=True):
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
            "exp_avg_sq": opt.exp_avg_sq.clone(), "steps": opt.steps, "lr": [g["lr"] for g in opt.param_groups], "global_step": eng.global_step}


def _same_state(got, want, what):
    for k in ("flat", "master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
    assert got["steps"] == want["steps"] and got["lr"] == want["lr"] and got["global_step"] == want["global_step"], what


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


def _record_ids(eng):
    """the batch ids the engine trains on, in order"""
    seen, inner = [], eng.train_step

    def train_step(batch, task, accum_steps=1):
        seen.append((task, tuple(batch["ids"])))
        return inner(batch, task, accum_steps=accum_steps)
    eng.train_step = train_step
    return seen


def _hand_loop(dev, steps, graphs, opts):
    """the loop every user wrote by hand: train_step over the loader's (name, batch) stream"""
    _seed_run(77)
    model, eng = _build(dev, 3, opts, graphs)
    losses, items = [], []
    it = iter(_loaders())
    for _ in range(steps):
        name, batch = next(it)
        out = eng.train_step(_to_dev(batch, dev), name.split("--")[0])
        losses.append((name, {k: v.detach().clone() for k, v in out.items()}))
        items.append((name.split("--")[0], tuple(batch["ids"])))
    st = _state(eng)
    norm = eng.optimizer.total_norm.clone()
    _teardown(model, eng)
    return st, losses, items, norm


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_fit_equals_the_hand_written_loop(dev, graphs):
    """two tasks on two named loaders, 6 optimizer steps: the parameter arena, fp32 masters, both moments, per-tensor step counts and every
    metered `last` are those of a loop of train_step calls over the same (name, batch) sequence"""
    from valor_amd.optim import get_lr_sched
    from valor_amd.train import Trainer
    want, losses, items, norm = _hand_loop(dev, 6, graphs, _opts(6))
    assert {n for n, _ in losses} == {TASK_A + "--dsetA", TASK_B + "--dsetB"}              # both tasks were drawn
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(6), graphs)
    seen = _record_ids(eng)
    logged = []
    out = Trainer(eng, _loaders(), log_fn=lambda s, sc: logged.append((s, sc)), log_every=1).fit()
    assert out["global_step"] == 6 and out["items"] == 6 and seen == items
    _same_state(_state(eng), want, "after 6 steps")
    by_step = {}
    for s, sc in logged:
        by_step.setdefault(s, sc)
    assert sorted(by_step) == [1, 2, 3, 4, 5, 6]
    for s in range(1, 7):
        name, ld = losses[s - 1]
        for k, v in ld.items():
            rec = by_step[s][f"loss_{name}/{k}"]
            assert rec["last"] == float(v), (s, name, k, rec, float(v))
        assert by_step[s]["gscale"]["count"] == s and by_step[s]["grad_norm"]["count"] == s and by_step[s]["gscale"]["nonfinite"] == 0
        assert by_step[s]["lr_ratio"] == float(get_lr_sched(s, _opts(6)))                 # host-known, rides with the snapshot
    assert by_step[6]["grad_norm"]["last"] == float(norm) == out["meter"]["grad_norm"]["last"]
    # the running fields against the restatement, from the loop's own losses
    from valor_amd.train import meter_host
    key = f"loss_{losses[0][0]}/total_loss"
    series = [float(ld["total_loss"]) for n, ld in losses if n == losses[0][0]]
    want_row = meter_host(series, np.float32(0.99), np.float32(1.0 - 0.99))
    got = out["meter"][key]
    assert [got[f] for f in ("last", "ema", "sum", "count", "min", "max", "nonfinite")] == [float(x) for x in want_row[:7]]
    _teardown(model, eng)


def test_exact_resume_through_the_driver(dev, tmp_path):
    """8 steps uninterrupted against fit to the checkpoint at step 4 (valid_steps = 5: (4 + 1) % 5 == 0), the run killed behind it, then a
    fresh model with other weights, a fresh optimizer, engine and loaders, a scrambled host RNG, and fit(resume=True) to step 8 -- with the
    prefetching loader on (it had pulled item 5 when the checkpoint was taken). Equal to the bit: parameters, masters, moments, step
    counts, the sequence of batch ids and the meter table. A checkpoint without its trainer file raises FileNotFoundError."""
    from valor_amd import checkpoint
    from valor_amd.train import Trainer, trainer_file
    quiet = lambda *a: None
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(8, valid_steps=5))
    ids_full = _record_ids(eng)
    tr = Trainer(eng, _loaders(), output_dir=str(tmp_path / "full"), log_fn=quiet)
    out = tr.fit()
    assert out["checkpoints"] == [4] and out["global_step"] == 8 and len(ids_full) == 8
    want, want_table, want_names = _state(eng), tr.meter.table[:len(tr.meter.names)].clone(), list(tr.meter.names)
    assert sorted(os.listdir(tmp_path / "full" / "ckpt")) == ["engine_step_4.rank0.pt", "model_step_4.pt", "optimizer_step_4.pt", "train_step_4.rank0.pt"]
    _teardown(model, eng)
    del model, eng, tr

    class Killed(Exception):
        pass
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(8, valid_steps=5))
    ids_head = _record_ids(eng)
    inner = eng.train_step

    def dies_after_four(batch, task, accum_steps=1):
        if eng.global_step == 4:
            raise Killed()
        return inner(batch, task, accum_steps=accum_steps)
    eng.train_step = dies_after_four
    run = str(tmp_path / "run")
    with pytest.raises(Killed):
        Trainer(eng, _loaders(), output_dir=run, log_fn=quiet).fit()
    _teardown(model, eng)                                   # close() waits for the non-blocking save
    assert checkpoint.latest_step(run) == 4 and os.path.exists(trainer_file(run, 4)) and ids_head == ids_full[:4]
    del model, eng

    _seed_run(4000)                                         # a process state in which only the load can make the runs agree
    model, eng = _build(dev, 11, _opts(8, valid_steps=5))
    assert not torch.equal(model.arena.flat, want["flat"])
    ids_tail = _record_ids(eng)
    tr = Trainer(eng, _loaders(), output_dir=run, log_fn=quiet)
    out = tr.fit(resume=True)
    assert out["global_step"] == 8 and out["items"] == 8 and ids_tail == ids_full[4:]
    assert len(set(ids_full)) == 8 and {t for t, _ in ids_full[4:]} == {TASK_A, TASK_B}
    _same_state(_state(eng), want, "resumed, step 8")
    assert tr.meter.names == want_names and torch.equal(_bits(tr.meter.table[:len(want_names)]), _bits(want_table))
    _teardown(model, eng)
    del model, eng, tr

    os.remove(trainer_file(run, 4))
    _seed_run(4000)
    model, eng = _build(dev, 11, _opts(8, valid_steps=5))
    before = model.arena.flat.clone()
    with pytest.raises(FileNotFoundError, match="train_step_4.rank0.pt"):
        Trainer(eng, _loaders(), output_dir=run, log_fn=quiet).fit(resume=True)
    assert torch.equal(model.arena.flat, before) and eng.global_step == 0                  # refused before anything was loaded
    _teardown(model, eng)


def test_validation_in_the_loop(dev, tmp_path):
    """a ret%tv validation loader of 4 clips at valid_steps = 2 (after the steps 1 and 3): the metrics of the last round equal
    evaluate.validate called by hand on the same weights, the model is back in train mode, decode holds no session, and with save_best
    best_ret%tv--....pt exists"""
    from valor_amd import evaluate, synth
    from valor_amd.train import Trainer
    spec = synth.tiny_spec()
    vb = []
    for i in range(2):
        b = synth.make_batch(spec, batch=2, frames=2, audio_slices=1, txt_len=32, seed=900 + i)
        b["ids"] = [f"v{2 * i + j}" for j in range(2)]
        b["ids_txt"] = list(b["ids"])
        vb.append(b)
    val = {"ret%tv--dsetV": vb}
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(4, valid_steps=2, save_best=True))
    model.__dict__["_decode_sessions"] = {"left over": object()}
    logged = []
    out = Trainer(eng, _loaders(), val_loaders=val, output_dir=str(tmp_path), log_fn=lambda s, sc: logged.append(s)).fit()
    assert out["global_step"] == 4 and sorted(out["validations"]) == [1, 3] and out["checkpoints"] == [1, 3]
    assert model.training and "_decode_sessions" not in model.__dict__
    name = "ret%tv--dsetV_t_v"
    assert os.path.exists(tmp_path / "ckpt" / f"best_{name}.pt")
    hist = out["best"][name]
    assert hist["best_step"] in (1, 3) and hist["best_value"] == max(hist["1"]["video_ravg"], hist["3"]["video_ravg"])
    assert logged[:2] == [1, 3]
    _teardown(model, eng)
    # by hand on the weights of step 3: the checkpoint of that step in a fresh model
    from valor_amd import checkpoint
    _seed_run(5)
    model2, eng2 = _build(dev, 11, _opts(4, valid_steps=2))
    assert checkpoint.resume_run(eng2, str(tmp_path)) == 3
    by_hand = evaluate.validate(model2, val)
    assert by_hand == out["validations"][3] and by_hand["ret%tv--dsetV"]["t_v"]["video_ravg"] == hist["3"]["video_ravg"]
    assert out["validations"][1] != {} and model2.training
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


def test_fit_adds_no_synchronisation(dev):
    """6 fit steps (log_every large, no validation) under torch.cuda.set_sync_debug_mode('warn') raise as many synchronisation warnings
    as the bare loop of train_step calls on the same batches"""
    from valor_amd.train import Trainer
    probe = torch.ones((), device=dev)
    if not _sync_warnings(lambda: probe.item()):
        pytest.skip("torch.cuda.set_sync_debug_mode('warn') is not live in this build: a deliberate .item() did not warn")
    batches = [(n, _to_dev(b, dev)) for n, b in (x for _, x in zip(range(6), iter(_loaders())))]

    def bare():
        for name, b in batches:
            eng.train_step(b, name.split("--")[0])

    _seed_run(77)
    model, eng = _build(dev, 3, _opts(6))
    loop = _sync_warnings(bare)
    torch.cuda.synchronize()
    _teardown(model, eng)
    _seed_run(77)
    model, eng = _build(dev, 3, _opts(6))
    tr = Trainer(eng, _loaders(), log_fn=lambda *a: None, log_every=10 ** 6)
    driver = _sync_warnings(tr.fit)
    torch.cuda.synchronize()
    print(f"synchronisation warnings: bare loop {len(loop)}, fit {len(driver)}")
    for m in sorted(set(loop + driver)):
        print(f"  loop {loop.count(m)} fit {driver.count(m)}: {m[:160]}")
    assert eng.global_step == 6 and len(driver) == len(loop), (len(driver), len(loop))
    _teardown(model, eng)
