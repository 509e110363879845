"""CPU: the host side of the training diagnostics (valor_amd/diagnostics.py) -- stats_host, the fp64 restatement of the two kernels' laws, on
hand-computed cases (exact element bounds, finite-only sums, inactive rows, the skipped step, the fold order), the delivered table's
by_module / nonfinite_tensors, the group names against model.params.optimizer_group, the argument refusals of the two entry points, and
the trainer's part on an engine that records its calls: the diagnostic keys reach the meter only when asked for, the non-finite record
is written."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

NAN, INF = float("nan"), float("inf")
F = {k: i for i, k in enumerate(("g_sumsq", "g_absmax", "g_nonfinite", "g_norm", "w_sumsq", "u_sumsq", "w_norm", "u_ratio"))}


def _arena():
    """chunk 4; tensors of 3, 4, 5, 2 elements on 1, 1, 2, 1 chunks; groups 0, 1, 0, 2; tensor 1 inactive; every pad element is NaN"""
    P = NAN
    grad = [3, -4, INF, P,   1, 1, 1, 1,   1, 2, -2, 4, 2, P, P, P,   6, -8, P, P]
    master = [1, 2, 2, P,    9, 9, 9, 9,   1, 1, 1, 1, 0, P, P, P,    3, 4, P, P]
    m = [1, 1, -1, P,        1, 1, 1, 1,   2, 0, 0, 0, 0, P, P, P,    1, 1, P, P]
    v = [4, 4, 4, P,         1, 1, 1, 1,   1, 1, 1, 1, 1, P, P, P,    1, 1, P, P]
    return dict(chunk_group=[0, -1, 0, 0, 2], chunk_tensor=[0, 1, 2, 2, 3], tensor_numel=[3, 4, 5, 2], ngroups=3, chunk=4,
                grad=np.array(grad, np.float32), master=np.array(master, np.float32), exp_avg=np.array(m, np.float32),
                exp_avg_sq=np.array(v, np.float32), chunk_bc=np.array([[0.5, 1.0], [1, 1], [1.0, 0.5], [1.0, 0.5], [1, 1]], np.float32),
                lr=[0.5, 0.25, 0.0], eps=0.0, norm_mul=0.5)


def test_stats_host_bounds_finite_sums_inactive_rows_and_groups():
    from valor_amd.diagnostics import stats_host
    ts, gs = stats_host(**_arena())
    assert ts.shape == (4, 8) and gs.shape == (3, 8) and ts.dtype == np.float64
    # tensor 0: 3 and -4 count, the inf is counted apart, the NaN pad is never seen
    assert ts[0, :4].tolist() == [25.0, 4.0, 1.0, 2.5]
    assert ts[1].tolist() == [0.0] * 8                                                  # inactive: zeros in every field
    assert ts[2, :4].tolist() == [29.0, 4.0, 0.0, np.sqrt(29.0) * 0.5]                  # the 5th element lives in the second chunk
    assert ts[3, :4].tolist() == [100.0, 8.0, 0.0, 5.0]
    # update fields: u = lr * bc[1] / bc[0] * m / (sqrt(v) + eps)
    assert ts[0, 4:].tolist() == [9.0, 0.75, 3.0, np.sqrt(0.75) / (3.0 + 1e-12)]        # u = 0.5 * 1 / 0.5 * (+-1 / 2) = +-0.5
    assert ts[2, 4:].tolist() == [4.0, 0.25, 2.0, 0.5 / (2.0 + 1e-12)]                  # u = 0.5 * 0.5 / 1 * 2 = 0.5 on one element
    assert ts[3, 4:].tolist() == [25.0, 0.0, 5.0, 0.0]                                  # lr 0: the group does not move
    assert gs[0].tolist() == [54.0, 4.0, 1.0, np.sqrt(54.0) * 0.5, 13.0, 1.0, np.sqrt(13.0), 1.0 / (np.sqrt(13.0) + 1e-12)]
    assert gs[1].tolist() == [0.0] * 8 and gs[2].tolist() == ts[3].tolist()
    # a call that was not asked for leaves its fields zero
    a = _arena()
    only_grad, _ = stats_host(**{k: a[k] for k in ("chunk_group", "chunk_tensor", "tensor_numel", "ngroups", "chunk", "grad", "norm_mul")})
    assert only_grad[:, :4].tolist() == ts[:, :4].tolist() and not only_grad[:, 4:].any()


def test_stats_host_skipped_step():
    from valor_amd.diagnostics import stats_host
    ts, gs = stats_host(**_arena())
    for bad in (NAN, INF, -INF):
        ts2, gs2 = stats_host(gscale=bad, **_arena())
        for a, b in ((ts, ts2), (gs, gs2)):
            assert not b[:, F["u_sumsq"]].any() and not b[:, F["u_ratio"]].any()
            assert b[:, [0, 1, 2, 3, 4, 6]].tolist() == a[:, [0, 1, 2, 3, 4, 6]].tolist()


def test_stats_host_folds_groups_in_tensor_order():
    """three tensors of one group with the sums of squares 1, 3 * 2^-55, 3 * 2^-55: in tensor order the fp64 fold stays at 1.0 (each
    addend is below half an ulp of 1); any order that adds the two small ones first gives 1 + 2^-52"""
    from valor_amd.diagnostics import stats_host
    small = [2.0 ** -28] * 6 + [NAN, NAN]
    grad = np.array([1.0, NAN, NAN, NAN] + small + small, np.float32)
    kw = dict(chunk_group=[0] * 5, chunk_tensor=[0, 1, 1, 2, 2], tensor_numel=[1, 6, 6], ngroups=1, chunk=4, grad=grad)
    ts, gs = stats_host(**kw)
    assert ts[:, 0].tolist() == [1.0, 3 * 2.0 ** -55, 3 * 2.0 ** -55]
    assert gs[0, 0] == 1.0 and (ts[1, 0] + ts[2, 0]) + ts[0, 0] == 1.0 + 2.0 ** -52
    # the other way round the large tensor comes last
    grad2 = np.array(small + small + [1.0, NAN, NAN, NAN], np.float32)
    _, gs2 = stats_host(**dict(kw, chunk_tensor=[0, 0, 1, 1, 2], tensor_numel=[6, 6, 1], grad=grad2))
    assert gs2[0, 0] == 1.0 + 2.0 ** -52


def test_tensor_table_by_module_and_nonfinite():
    from valor_amd.diagnostics import TensorTable
    names = ["enc.layer.0.w", "enc.layer.0.b", "enc.layer.1.w", "head.w"]
    rows = np.zeros((4, 8))
    rows[:, F["g_sumsq"]] = [9, 16, 144, 4]
    rows[:, F["g_absmax"]] = [3, 2, 7, 2]
    rows[:, F["g_nonfinite"]] = [0, 2, 0, 1]
    rows[:, F["w_sumsq"]] = [1, 3, 4, 0]
    rows[:, F["u_sumsq"]] = [0.25, 0.75, 0.0, 0.0]
    t = TensorTable(12, names, rows, norm_mul=0.5)
    assert t.step == 12 and t.nonfinite_tensors() == ["enc.layer.0.b", "head.w"]
    assert t.by_tensor()["enc.layer.1.w"]["g_absmax"] == 7.0 and list(t.by_tensor()) == names
    top = t.by_module(1)
    assert list(top) == ["enc", "head"]
    assert top["enc"] == {"g_sumsq": 169.0, "g_absmax": 7.0, "g_nonfinite": 2.0, "g_norm": 6.5, "w_sumsq": 8.0, "u_sumsq": 1.0,
                          "w_norm": np.sqrt(8.0), "u_ratio": 1.0 / (np.sqrt(8.0) + 1e-12)}
    assert top["head"]["g_norm"] == 1.0 and top["head"]["u_ratio"] == 0.0 and top["head"]["w_norm"] == 0.0
    deep = t.by_module(3)
    assert list(deep) == ["enc.layer.0", "enc.layer.1", "head.w"]
    assert deep["enc.layer.0"]["g_sumsq"] == 25.0 and deep["enc.layer.0"]["g_norm"] == 2.5 and deep["enc.layer.0"]["u_ratio"] == 1.0 / (2.0 + 1e-12)


def test_group_names_follow_optimizer_group():
    from valor_amd.diagnostics import GROUP_NAMES
    from valor_amd.model.params import optimizer_group
    assert len(GROUP_NAMES) == 10 == len(set(GROUP_NAMES))
    cases = {"multimodal_encoder.encoder.layer.0.attention.self.query.weight": "basic_decay",
             "multimodal_encoder.encoder.layer.0.attention.output.LayerNorm.weight": "basic_no_decay",
             "clip_model.visual.transformer.resblocks.0.attn.in_proj_weight": "clip_visual_decay",
             "clip_model.visual.transformer.resblocks.0.attn.in_proj_bias": "clip_visual_no_decay",
             "clip_model.transformer.resblocks.0.mlp.c_fc.weight": "clip_text_decay",
             "clip_model.ln_final.bias": "clip_text_no_decay",
             "multimodal_encoder.decoder.layer.1.output.dense.weight": "decoder_decay",
             "multimodal_encoder.decoder.layer.1.output.dense.bias": "decoder_no_decay"}
    for ref, want in cases.items():
        assert GROUP_NAMES[optimizer_group(ref)] == want, ref
    assert GROUP_NAMES[optimizer_group("contra_head_t.weight", ("contra_head",))] == "new_decay"
    assert GROUP_NAMES[optimizer_group("contra_head_t.bias", ("contra_head",))] == "new_no_decay"


def test_stats_argument_validation_without_gpu():
    """both entry points refuse before any launch; n = 0 is a no-op"""
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_float * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    lr = (ctypes.c_float * 17)(*([1e-3] * 17))

    def grad(n=2048, ntensors=2, ngroups=3, dtype=0, **kw):
        a = dict(grad=p, cg=p, ct=p, numel=p, scratch=p, ts=p, gs=p)
        a.update(kw)
        return so.valor_arena_grad_stats(None, dtype, a["grad"], a["cg"], a["ct"], a["numel"], ntensors, n, ngroups, 1.0, a["scratch"], a["ts"], a["gs"])

    def upd(n=2048, ntensors=2, ngroups=3, lr_=lr, **kw):
        a = dict(master=p, m=p, v=p, cg=p, ct=p, bc=p, numel=p, gscale=p, scratch=p, ts=p, gs=p)
        a.update(kw)
        return so.valor_arena_update_stats(None, a["master"], a["m"], a["v"], a["cg"], a["ct"], a["bc"], a["numel"], ntensors, n, lr_, ngroups, 1e-6,
                                           a["gscale"], a["scratch"], a["ts"], a["gs"])

    for f, ptrs in ((grad, ("grad", "cg", "ct", "numel", "scratch", "ts", "gs")),
                    (upd, ("master", "m", "v", "cg", "ct", "bc", "numel", "scratch", "ts", "gs"))):
        assert f(n=1000) == -1 and f(n=2049) == -1 and f(n=-1024) == -1
        assert f(ntensors=0) == -1 and f(ntensors=-2) == -1
        assert f(ngroups=0) == -1 and f(ngroups=17) == -1
        for k in ptrs:
            assert f(**{k: None}) == -1, k
        for k in ("scratch", "ts", "gs"):
            assert f(**{k: p + 4}) == -1 and f(**{k: p + 8}) == -1, k
        assert f(ct=p + 2) == -1 and f(numel=p + 4) == -1
        assert f(n=0) == 0 and f(n=0, ngroups=0, ntensors=0) == 0
    assert grad(dtype=7) == -1 and grad(grad=p + 8) == -1
    assert upd(master=p + 4) == -1 and upd(m=p + 8) == -1 and upd(v=p + 4) == -1 and upd(bc=p + 4) == -1 and upd(gscale=p + 2) == -1
    assert upd(lr_=None) == -1


def test_diagnostics_has_no_host_path():
    from valor_amd import kernels, lib
    z = torch.zeros(1024)
    with pytest.raises(lib.ValorHipError):
        kernels.arena_grad_stats(z, torch.zeros(1, dtype=torch.int8), torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int64), 1.0,
                                 torch.zeros(16), torch.zeros(1, 8), torch.zeros(1, 8))


# ------------------------------------------------------------------------------------------------------------------ the trainer
class Loader:
    def __init__(self, tag, n):
        self.tag, self.n = tag, n

    def __iter__(self):
        for i in range(self.n):
            yield {"ids": [self.tag, i]}


class RecordingMeter:
    device = None

    def __init__(self):
        self.updates = []

    def update(self, name, loss_dict, extra=None):
        self.updates.append(None if extra is None else sorted(extra))

    def snapshot(self, step=None, host=None):
        pass

    def poll(self):
        return []

    def flush(self, step=None, host=None):
        return [(step, dict(host or {}))]


class FakeDiagnostics:
    """what the trainer uses of a Diagnostics: fresh / table_step, scalars(), snapshot(), poll(), flush(); the engine flips `fresh` on
    every second step like every=2; the table of step 3 shows two tensors with non-finite gradients"""

    def __init__(self):
        self.fresh, self.table_step, self.snaps, self.out = False, None, [], []

    def scalars(self):
        return {"grad_norm/basic_decay": torch.zeros(()), "grad_absmax/basic_decay": torch.zeros(())}

    def snapshot(self, step=None):
        from valor_amd.diagnostics import TensorTable
        self.snaps.append(step)
        rows = np.zeros((3, 8))
        if step == 3:
            rows[[0, 2], F["g_nonfinite"]] = [1, 5]
        self.out.append(TensorTable(step, ["a.w", "a.b", "c.w"], rows))

    def poll(self):
        out, self.out = self.out, []
        return out

    def flush(self, step=None):
        self.snapshot(step)
        return self.poll()


def _engine(diag_holder):
    from valor_amd.optim import FusedAdamW

    class Opt(FusedAdamW):
        def __init__(self):
            self.total_norm, self.gscale = torch.zeros(()), torch.ones(())

    class Engine:
        diagnostics = None

        def __init__(self):
            self.opts = SimpleNamespace(num_train_steps=6, warmup_ratio=0.1, scheduler="warmup_linear")
            self.optimizer, self.global_step = Opt(), 0
            self.model = SimpleNamespace()

        def train_step(self, batch, task, accum_steps=1):
            d = self.diagnostics
            if d is not None:
                d.fresh = self.global_step % 2 == 0
                if d.fresh:
                    d.table_step = self.global_step
            self.global_step += 1
            return {"total_loss": torch.zeros(())}
    return Engine()


def test_trainer_meters_diagnostics_only_when_asked_and_logs_nonfinite_tensors():
    from valor_amd.train import MetaLoader, Trainer
    loaders = lambda: MetaLoader({"pt_mlm%tv--d": Loader("a", 4)}, seed=1)
    # without: the extras are grad_norm and gscale, nothing else reaches the sink
    eng, meter, logged = _engine(None), RecordingMeter(), []
    Trainer(eng, loaders(), log_fn=lambda s, sc: logged.append((s, sc)), log_every=1, meter=meter, prefetch=False).fit()
    assert eng.diagnostics is None and meter.updates == [["grad_norm", "gscale"]] * 6
    assert all("nonfinite_tensors" not in sc for _, sc in logged)
    # with: the steps that wrote the table add its keys; the snapshot of step 3 produces ONE record naming the tensors
    eng, meter, logged, diag = _engine(None), RecordingMeter(), [], FakeDiagnostics()
    tr = Trainer(eng, loaders(), log_fn=lambda s, sc: logged.append((s, sc)), log_every=1, meter=meter, prefetch=False, diagnostics=diag)
    tr.fit()
    assert eng.diagnostics is diag and tr.diagnostics is diag
    with_keys = ["grad_absmax/basic_decay", "grad_norm", "grad_norm/basic_decay", "gscale"]
    assert meter.updates == [with_keys, ["grad_norm", "gscale"]] * 3
    assert diag.snaps == [1, 2, 3, 4, 5, 6, 6]                                  # the logging cadence, then the final flush
    assert [(s, sc) for s, sc in logged if "nonfinite_tensors" in sc] == [(3, {"nonfinite_tensors": ["a.w", "c.w"]})]


def test_trainer_reads_the_diagnostics_options(monkeypatch):
    from valor_amd import diagnostics, train
    built = []

    class Stub(FakeDiagnostics):
        def __init__(self, optimizer, level="grad", every=1):
            super().__init__()
            built.append((optimizer, level, every))
    monkeypatch.setattr(diagnostics, "Diagnostics", Stub)
    loaders = train.MetaLoader({"pt_mlm%tv--d": Loader("a", 4)}, seed=1)
    eng = _engine(None)
    assert train.Trainer(eng, loaders, meter=RecordingMeter()).diagnostics is None and not built
    eng.opts.diag_level, eng.opts.diag_every = "full", 4
    tr = train.Trainer(eng, loaders, meter=RecordingMeter())
    assert built == [(eng.optimizer, "full", 4)] and eng.diagnostics is tr.diagnostics
    eng2 = _engine(None)
    train.Trainer(eng2, loaders, meter=RecordingMeter(), diagnostics=True)
    train.Trainer(eng2, loaders, meter=RecordingMeter(), diagnostics="full")
    assert built[1:] == [(eng2.optimizer, "grad", 1), (eng2.optimizer, "full", 1)]
    monkeypatch.undo()
    with pytest.raises(ValueError, match="level"):
        diagnostics.Diagnostics(None, level="all")
    with pytest.raises(ValueError, match="every"):
        diagnostics.Diagnostics(None, every=0)
