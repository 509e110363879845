"""CPU: the training driver's host side (valor_amd/train.py) -- the laws of the task-mixing loaders (data/loader.py:22-124 restated), their
restorable position, the distributed task draw, the numpy restatement of the device meter's law, the argument refusals of
valor_meter_update, and Trainer.fit's control flow (train_utils.py:277-398) on an engine that records its calls. All comparisons are ==."""
import ctypes
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ loaders
class Sampler:
    def __init__(self):
        self.epochs = []
        self.epoch = 0

    def set_epoch(self, e):
        self.epochs.append(e)
        self.epoch = e


class Loader:
    """`n` batches per epoch, batch i of epoch e has the ids [tag, e, i]: a function of (epoch, index)"""

    def __init__(self, tag, n, with_skip=False):
        self.tag, self.n, self.sampler = tag, n, Sampler()
        self.skipped = []
        if with_skip:
            self.skip = self._skip

    def _gen(self, first):
        e = self.sampler.epoch
        for i in range(first, self.n):
            yield {"ids": [self.tag, e, i]}

    def __iter__(self):
        return self._gen(0)

    def _skip(self, k):
        self.skipped.append(k)
        return self._gen(k)


def _take(loader, n, it=None):
    it = iter(loader) if it is None else it
    return [(name, tuple(b["ids"])) for name, b in (next(it) for _ in range(n))]


def test_meta_loader_laws():
    """against a restatement of data/loader.py:75-124 on the same generator: the pool holds every name `ratio` times, a task is drawn
    every accum_steps yields and kept in between, exhaustion bumps the shared epoch and calls set_epoch on that loader's sampler"""
    from valor_amd.train import MetaLoader
    A, B = Loader("a", 3), Loader("b", 2)
    ml = MetaLoader({"t1--a": (A, 3), "t2--b": B}, accum_steps=2, seed=5)
    assert ml.sampling_pools == ["t1--a"] * 3 + ["t2--b"] and ml.ndata == 2
    got = _take(ml, 24)
    rng = random.Random(5)
    pools, left, cur = ml.sampling_pools, {"t1--a": 3, "t2--b": 2}, {"t1--a": [0, 0], "t2--b": [0, 0]}
    want, epoch, task, sizes = [], 0, None, {"t1--a": 3, "t2--b": 2}
    for step in range(24):
        if step % 2 == 0:
            task = rng.choice(pools)
        if cur[task][1] == sizes[task]:
            epoch += 1
            cur[task] = [epoch, 0]
        want.append((task, (task[-1], cur[task][0], cur[task][1])))
        cur[task][1] += 1
    assert got == want
    assert all(got[i][0] == got[i + 1][0] for i in range(0, 24, 2))                    # the task is kept for accum_steps yields
    assert {n for n, _ in got} == {"t1--a", "t2--b"}
    assert ml.epoch == epoch >= 2 and sorted(A.sampler.epochs + B.sampler.epochs) == list(range(1, epoch + 1))
    assert ml.step == ml.yielded == 24


def test_accum_loader_is_round_robin():
    from valor_amd.train import AccumMetaLoader
    A, B, C = Loader("a", 2), Loader("b", 5), Loader("c", 5)
    al = AccumMetaLoader({"x--a": A, "y--b": B, "z--c": (C, 4)})
    assert al.ndata == 3
    got = _take(al, 9)
    assert [n for n, _ in got] == ["x--a", "y--b", "z--c"] * 3
    assert [i for n, i in got if n == "x--a"] == [("a", 0, 0), ("a", 0, 1), ("a", 1, 0)] and A.sampler.epochs == [1]
    assert B.sampler.epochs == [] and [i for n, i in got if n == "y--b"] == [("b", 0, 0), ("b", 0, 1), ("b", 0, 2)]


def test_the_draw_leaves_the_global_generator_alone():
    from valor_amd.train import MetaLoader
    random.seed(3)
    before = random.getstate()
    _take(MetaLoader({"t--a": Loader("a", 3), "t--b": Loader("b", 3)}, seed=1), 10)
    assert random.getstate() == before


@pytest.mark.parametrize("kind", ["meta", "accum"])
@pytest.mark.parametrize("behind", [0, 1, 3])
def test_loader_position(kind, behind):
    """state_dict(consumed=n) -> a fresh loader -> the same (name, ids) sequence from item n, for n = yielded, one less, three less (a
    prefetcher is one ahead); with and without loader.skip; through epoch roll-overs and in the middle of a kept task"""
    from valor_amd.train import AccumMetaLoader, MetaLoader

    def make(with_skip=False):
        ls = {"t1--a": (Loader("a", 3, with_skip), 2), "t2--b": Loader("b", 4, with_skip)}
        return (MetaLoader(ls, accum_steps=3, seed=9) if kind == "meta" else AccumMetaLoader(ls)), ls

    ref, _ = make()
    want = _take(ref, 40)
    for yielded in (5, 11, 22):
        src, _ = make()
        assert _take(src, yielded) == want[:yielded]
        n = yielded - behind
        sd = src.state_dict(consumed=n)
        assert sd["yielded"] == n
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"valor_loader_state_{os.getpid()}.pt")
        torch.save(sd, path)
        sd = torch.load(path, map_location="cpu", weights_only=True)          # what the trainer's file goes through
        os.remove(path)
        for with_skip in (False, True):
            dst, ls = make(with_skip)
            dst.load_state_dict(sd)
            assert _take(dst, 40 - n) == want[n:], (yielded, n, with_skip)
            assert dst.yielded == 40
            if with_skip:
                assert all(len((v[0] if isinstance(v, tuple) else v).skipped) == 1 for v in ls.values())


def test_loader_position_outside_the_history():
    from valor_amd.train import MetaLoader
    ml = MetaLoader({"t--a": Loader("a", 3)}, seed=0)
    _take(ml, 10)
    assert ml.state_dict(consumed=6)["yielded"] == 6
    for n in (5, 0, 11):
        with pytest.raises(ValueError, match="history"):
            ml.state_dict(consumed=n)
    with pytest.raises(ValueError):
        MetaLoader({"t--a": Loader("a", 3), "t--b": Loader("b", 3)}).load_state_dict(ml.state_dict())


def _draw_case(rank, world):
    from valor_amd.train import MetaLoader
    ml = MetaLoader({"t1--a": Loader("a", 50), "t2--b": Loader("b", 50), "t3--c": Loader("c", 50)}, accum_steps=2, distributed=True,
                    seed=100 + rank)
    return [n for n, _ in _take(ml, 30)]


def test_distributed_task_draw():
    """world 2 over gloo: both ranks train the same task sequence although their local seeds differ (rank 0's draw is broadcast)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_dist_cpu import _run
    from valor_amd.train import MetaLoader
    r = _run(_draw_case, 2)
    assert r[0] == r[1] and len(set(r[0])) == 3
    local = [n for n, _ in _take(MetaLoader({"t1--a": Loader("a", 50), "t2--b": Loader("b", 50), "t3--c": Loader("c", 50)}, accum_steps=2,
                                            seed=101), 30)]
    assert local != r[1]                                   # rank 1's own draws would have differed


# ------------------------------------------------------------------------------------------------------------------ the meter
def test_meter_host_against_a_hand_computed_sequence():
    from valor_amd.train import ROW_INIT, meter_host
    f = np.float32
    keep, take = f(0.99), f(1 - 0.99)
    nan, inf = float("nan"), float("inf")
    r = meter_host([], keep, take)
    assert r.dtype == np.float32 and r.tolist() == list(ROW_INIT) == [0, 0, 0, 0, inf, -inf, 0, 0]
    r = meter_host([2.5], keep, take)
    assert r.tolist() == [2.5, 2.5, 2.5, 1, 2.5, 2.5, 0, 0]                          # the first value as it is; min / max leave +-inf
    r = meter_host([nan], keep, take)
    assert np.isnan(r[0]) and r[1:].tolist() == [0, 0, 0, inf, -inf, 1, 0]           # only last and nonfinite move
    r = meter_host([nan, -inf, 4.0], keep, take)
    assert r.tolist() == [4, 4, 4, 1, 4, 4, 2, 0]                                   # the first FINITE value starts the average
    r = meter_host([1.0, nan, 3.0, inf, -2.0], keep, take)
    e1 = f(f(f(3.0) * take) + f(f(1.0) * keep))
    e2 = f(f(f(-2.0) * take) + f(e1 * keep))
    assert r.tolist() == [-2.0, float(e2), 2.0, 3.0, -2.0, 3.0, 2.0, 0.0]
    assert float(e1) == 1.0199999809265137 and abs(float(e2) - 0.9898) < 1e-6
    again = meter_host([3.0, inf, -2.0], keep, take, row=meter_host([1.0, nan], keep, take))        # a row continues
    assert again.tobytes() == r.tobytes()
    # an inf does not stick in the average (the reference skips only NaN)
    assert np.isfinite(meter_host([1.0, inf, 2.0], keep, take)[1])


def test_meter_update_argument_validation_without_gpu():
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    table = (p + 15) & ~15

    def meter(n=2, rows=4, tab=table, srcs=None, idx=None, null_src=False, null_idx=False):
        srcs = [table + 32, table + 36] + [table + 40 + 4 * i for i in range(40)] if srcs is None else srcs
        idx = list(range(40)) if idx is None else idx
        m = max(n, 1)
        s = (ctypes.c_void_p * m)(*srcs[:m])
        r = (ctypes.c_int32 * m)(*idx[:m])
        return so.valor_meter_update(None, tab, rows, None if null_src else s, None if null_idx else r, n, 0.99, 0.01)

    assert meter(rows=0) == -1 and meter(rows=-3) == -1
    assert meter(n=-1) == -1 and meter(n=33, rows=64) == -1
    assert meter(tab=None) == -1 and meter(null_src=True) == -1 and meter(null_idx=True) == -1
    assert meter(tab=table + 4) == -1                                     # the rows are read as 16-byte vectors
    assert meter(srcs=[table + 32, None]) == -1 and meter(srcs=[table + 32, table + 38]) == -1
    assert meter(idx=[0, 4]) == -1 and meter(idx=[-1, 2]) == -1           # a row outside the table
    assert meter(idx=[3, 3]) == -1                                        # two sources on one row would race
    assert meter(n=3, rows=64, idx=[5, 9, 5]) == -1
    assert meter(n=0) == 0 and meter(n=0, rows=0, tab=None) == 0          # nothing to fold: no-op


def test_loss_meter_has_no_host_path():
    from valor_amd import lib
    from valor_amd.train import LossMeter
    m = LossMeter("cpu")
    with pytest.raises(lib.ValorHipError):
        m.update("t--d", {"x": torch.zeros(())})


# ------------------------------------------------------------------------------------------------------------------ the loop
class FakeMeter:
    device = None

    def __init__(self):
        self.updates, self.flushes, self.loaded = [], 0, None

    def update(self, name, loss_dict, extra=None):
        self.updates.append((name, sorted(loss_dict), None if extra is None else sorted(extra)))

    def snapshot(self, step=None, host=None):
        pass

    def poll(self):
        return []

    def flush(self, step=None, host=None):
        self.flushes += 1
        return [(step, dict(host or {}, flushes=self.flushes))]

    def state_dict(self):
        return {"updates": len(self.updates)}

    def load_state_dict(self, sd):
        self.loaded = sd


def _fake_engine(contra_window=False, **kw):
    from valor_amd.optim import FusedAdamW

    class Opt(FusedAdamW):
        def __init__(self):
            self.total_norm, self.gscale = torch.zeros(()), torch.ones(())

    class Engine:
        def __init__(self):
            self.opts = SimpleNamespace(num_train_steps=12, warmup_ratio=0.1, scheduler="warmup_linear", **kw)
            self.optimizer, self.global_step, self.calls, self._micro = Opt(), 0, [], 0
            self.contra_window = contra_window
            self.model = SimpleNamespace(state_dict=lambda: {"w": torch.full((2,), float(self.global_step))}, _decode_sessions={"k": 1})

        def train_step(self, batch, task, accum_steps=1):
            self._micro += 1
            if self._micro % accum_steps == 0:
                self.global_step += 1
            self.calls.append(("step", task, tuple(batch["ids"]), accum_steps, self.global_step))
            return {"a_loss": torch.zeros(()), "total_loss": torch.zeros(())}

        def train_window(self, batches, task):
            self.global_step += 1
            self.calls.append(("window", task, tuple(tuple(b["ids"]) for b in batches), self.global_step))
            return {"contra_loss": torch.zeros(()), "total_loss": torch.zeros(())}
    return Engine()


@pytest.fixture
def hooks(monkeypatch):
    """evaluate.validate / decode.release_sessions / checkpoint.save_run as the trainer calls them, recorded in order"""
    from valor_amd import train
    log = []
    metrics = {}

    def validate(model, val_loaders, *, annotations=None, output_dir=None, global_step=0, **kw):
        log.append(("validate", global_step, dict(getattr(model, "_decode_sessions", None) or {}) != {}))
        return {key: {"t_v": {"video_ravg": metrics.get(global_step, 1.0), "video_recall": "r"}} for key in val_loaders}

    real_release = train.decode.release_sessions

    def release(model):
        log.append(("release",))
        real_release(model)

    def save_run(engine, output_dir, step=None, blocking=True):
        log.append(("save", engine.global_step, blocking))
        return SimpleNamespace(done=lambda: True, wait=lambda: engine.global_step, step=engine.global_step)

    monkeypatch.setattr(train.evaluate, "validate", validate)
    monkeypatch.setattr(train.decode, "release_sessions", release)
    monkeypatch.setattr(train.checkpoint, "save_run", save_run)
    return SimpleNamespace(log=log, metrics=metrics)


def _loaders(accum_steps=1, seed=2):
    from valor_amd.train import MetaLoader
    return MetaLoader({"pt_contra%tv--dsetA": Loader("a", 5), "pt_mlm%tv--dsetB": Loader("b", 3)}, accum_steps=accum_steps, seed=seed)


def test_fit_validates_checkpoints_and_stops(hooks, tmp_path):
    """num_train_steps = 12, valid_steps = 3: validation and checkpoint after the steps 2, 5, 8, 11 ((global_step + 1) % valid_steps == 0,
    train_utils.py:368), in the order flush -> validate -> release -> save(non-blocking); 12 items, every one an optimizer step; the
    trainer's file of the last checkpoint is the only one left; best_*.pt only written on >= (train_utils.py:383)"""
    from valor_amd import train
    eng = _fake_engine(valid_steps=3, save_best=True)
    meter = FakeMeter()
    hooks.metrics.update({2: 5.0, 5: 4.0, 8: 5.0, 11: 1.0})
    logged = []
    best_mtime = {}
    real_write = train.checkpoint._write
    writes = []

    def write(obj, path):
        writes.append((eng.global_step, os.path.basename(path)))
        real_write(obj, path)
    train.checkpoint._write = write
    try:
        tr = train.Trainer(eng, _loaders(), val_loaders={"ret%tv--dsetV": [1]}, output_dir=str(tmp_path), log_fn=lambda s, sc: logged.append((s, sc)),
                           meter=meter)
        out = tr.fit()
    finally:
        train.checkpoint._write = real_write
    want_items = _take(_loaders(), 12)
    assert [(c[1] + "--" + ("dsetA" if c[2][0] == "a" else "dsetB"), c[2]) for c in eng.calls] == want_items
    assert [c[1] for c in eng.calls] == [n.split("--")[0] for n, _ in want_items] and all(c[0] == "step" and c[3] == 1 for c in eng.calls)
    assert out["global_step"] == 12 == eng.global_step and out["items"] == 12 and out["checkpoints"] == [2, 5, 8, 11]
    assert hooks.log == [x for s in (2, 5, 8, 11) for x in (("validate", s, True if s == 2 else False), ("release",), ("save", s, False))]
    assert meter.flushes == 5 and [s for s, _ in logged] == [2, 5, 8, 11, 12]                 # one flush per validation + the final one
    assert all(u[2] == ["grad_norm", "gscale"] and u[1] == ["a_loss", "total_loss"] for u in meter.updates) and len(meter.updates) == 12
    assert meter.updates[0][0] == want_items[0][0]
    name = "ret%tv--dsetV_t_v"
    assert out["best"][name]["best_step"] == 8 and out["best"][name]["best_value"] == 5.0     # 5.0 at step 8 ties step 2: >= moves it
    assert [w for w in writes if w[1].startswith("best_")] == [(2, f"best_{name}.pt"), (8, f"best_{name}.pt")]
    assert torch.equal(torch.load(tmp_path / "ckpt" / f"best_{name}.pt")["w"], torch.full((2,), 8.0))
    assert sorted(os.listdir(tmp_path / "ckpt")) == [f"best_{name}.pt", "train_step_11.rank0.pt"]
    assert [w for w in writes if w[1].startswith("train_")] == [(s, f"train_step_{s}.rank0.pt") for s in (2, 5, 8, 11)]
    sd = torch.load(train.trainer_file(str(tmp_path), 11), weights_only=True)
    assert sd["consumed"] == 11 and sd["loader"][0]["yielded"] == 11 and sd["metric_logger"][name]["best_step"] == 8
    # the position in the file continues the stream where the engine stopped
    fresh = _loaders()
    fresh.load_state_dict(sd["loader"][0])
    assert _take(fresh, 1) == want_items[11:12]


def test_fit_keeps_old_trainer_files_when_asked(hooks, tmp_path):
    from valor_amd import train
    eng = _fake_engine(valid_steps=3, remove_before_ckpt=False)
    train.Trainer(eng, _loaders(), output_dir=str(tmp_path), log_fn=lambda *a: None, meter=FakeMeter()).fit()
    assert sorted(os.listdir(tmp_path / "ckpt")) == sorted(f"train_step_{s}.rank0.pt" for s in (2, 5, 8, 11))
    assert [x for x in hooks.log if x[0] == "validate"] == []                                  # no validation loaders: checkpoints only


def test_fit_valid_freq_and_no_validation(hooks):
    from valor_amd import train
    eng = _fake_engine(valid_freq=3)                        # 12 // 3 - 1 = 3 (train_utils.py:512)
    assert train.Trainer(eng, _loaders(), meter=FakeMeter()).valid_steps == 3
    eng = _fake_engine()
    tr = train.Trainer(eng, _loaders(), val_loaders={"ret%tv--v": [1]}, meter=FakeMeter())
    assert tr.valid_steps == 0 and tr.fit()["global_step"] == 12 and hooks.log == []


def test_fit_accum_grouping(hooks):
    """dataset_mix_type='accum': train_step(batch, task, accum_steps=ndata), an optimizer step every ndata items; grad_norm / gscale are
    metered at the closing micro-step only; validation once per optimizer step"""
    from valor_amd import train
    from valor_amd.train import AccumMetaLoader
    eng = _fake_engine(valid_steps=3, dataset_mix_type="accum")
    eng.opts.num_train_steps = 6
    meter = FakeMeter()
    al = AccumMetaLoader({"pt_contra%tv--dsetA": Loader("a", 5), "pt_mlm%tv--dsetB": Loader("b", 3)})
    out = train.Trainer(eng, al, val_loaders={"ret%tv--v": [1]}, meter=meter).fit()
    assert out["items"] == 12 and out["global_step"] == 6 and all(c[3] == 2 for c in eng.calls)
    assert [c[1] for c in eng.calls] == ["pt_contra%tv", "pt_mlm%tv"] * 6
    assert [u[2] for u in meter.updates] == [None, ["grad_norm", "gscale"]] * 6
    assert [x[1] for x in hooks.log if x[0] == "validate"] == [2, 5]


def test_fit_window_grouping(hooks):
    from valor_amd import train
    eng = _fake_engine(contra_window=True)
    eng.opts.num_train_steps = 5
    out = train.Trainer(eng, _loaders(accum_steps=3), window=3, meter=FakeMeter()).fit()
    want = _take(_loaders(accum_steps=3), 15)
    assert out["items"] == 15 and out["global_step"] == 5 and len(eng.calls) == 5
    for i, c in enumerate(eng.calls):
        assert c[0] == "window" and c[1] == want[3 * i][0].split("--")[0] and list(c[2]) == [ids for _, ids in want[3 * i:3 * i + 3]]
    with pytest.raises(ValueError, match="contra_window"):
        train.Trainer(_fake_engine(), _loaders(accum_steps=3), window=3, meter=FakeMeter())
    with pytest.raises(ValueError, match="mixes tasks"):
        train.Trainer(_fake_engine(contra_window=True), _loaders(accum_steps=1, seed=2), window=3, meter=FakeMeter()).fit()


def test_fit_first_eval_and_zero_shot(hooks):
    from valor_amd import train
    eng = _fake_engine(first_eval=True, zero_shot=True)
    out = train.Trainer(eng, _loaders(), val_loaders={"ret%tv--v": [1]}, meter=FakeMeter()).fit()
    assert out["global_step"] == 0 and eng.calls == [] and list(out["validations"]) == [0]
    assert hooks.log == [("validate", 0, True), ("release",)]
    del hooks.log[:]
    eng = _fake_engine(first_eval=True)
    eng.opts.num_train_steps = 2
    out = train.Trainer(eng, _loaders(), val_loaders={"ret%tv--v": [1]}, meter=FakeMeter()).fit()
    assert out["global_step"] == 2 and hooks.log[0] == ("validate", 0, True) and len(eng.calls) == 2


def test_fit_refuses_other_optimizers_and_missing_trainer_file(hooks, tmp_path):
    from valor_amd import train
    eng = _fake_engine()
    eng.optimizer = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1)
    with pytest.raises(TypeError, match="fused AdamW"):
        train.Trainer(eng, _loaders(), meter=FakeMeter())
    # a complete checkpoint of the three run files without the trainer's own
    os.makedirs(tmp_path / "ckpt")
    for n in ("model_step_4.pt", "optimizer_step_4.pt", "engine_step_4.rank0.pt"):
        torch.save({}, tmp_path / "ckpt" / n)
    with pytest.raises(FileNotFoundError, match="train_step_4.rank0.pt"):
        train.Trainer(_fake_engine(), _loaders(), output_dir=str(tmp_path), log_fn=lambda *a: None, meter=FakeMeter()).fit(resume=True)


def test_jsonl_sink(tmp_path):
    import json
    from valor_amd.train import JsonlSink
    sink = JsonlSink(str(tmp_path))
    sink(3, {"lr_ratio": 0.5, "loss_t--d/x": {"last": 1.0, "ema": 2.0}})
    sink(4, {"lr_ratio": 0.25})
    rows = [json.loads(l) for l in open(tmp_path / "log" / "train.jsonl")]
    assert rows == [{"lr_ratio": 0.5, "loss_t--d/x": {"last": 1.0, "ema": 2.0}, "step": 3}, {"lr_ratio": 0.25, "step": 4}]
