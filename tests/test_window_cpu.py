"""CPU: the host side of the window step (TrainEngine.train_window -- the contrastive loss over a whole accumulation window): the
argument rules, the window bank's slicing on plain tensors, the dropout-window handle of ops.DropoutState in host mode and the
bookkeeping of model.valor.WindowPass. Nothing here launches a kernel: the models are built on the CPU (tables and arenas only).
The device side -- reference semantics, replay, one evaluation per window -- is tests/test_window_gpu.py."""
from types import SimpleNamespace

import pytest
import torch

from valor_amd import engine as E
from valor_amd import ops, synth
from valor_amd.engine import TrainEngine
from valor_amd.model.valor import VALOR, WindowPass

TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"


@pytest.fixture(autouse=True)
def host_mode():
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)


@pytest.fixture(scope="module")
def eng():
    spec = synth.tiny_spec()
    model = VALOR({"dropout": 0.0}, spec=spec, dtype=torch.float32, device="cpu")
    o = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, betas=[0.9, 0.98], num_train_steps=100, warmup_ratio=0.1)
    return TrainEngine(model, o, manage_gc=False)


def _batches(sizes):
    spec = synth.tiny_spec()
    return [synth.make_batch(spec, batch=n, frames=2, audio_slices=1, txt_len=32, seed=4 + i) for i, n in enumerate(sizes)]


def test_unequal_micro_batches_are_refused(eng):
    with pytest.raises(ValueError, match="unequal"):
        eng.train_window(_batches((2, 3)), TASK)
    with pytest.raises(ValueError, match="no micro-batches"):
        eng.train_window([], TASK)
    assert eng.global_step == 0


def test_world_above_one_is_not_implemented(eng, monkeypatch):
    monkeypatch.setattr(eng, "world", 2)
    with pytest.raises(NotImplementedError, match="world > 1"):
        eng.train_window(_batches((2, 2)), TASK)


def test_an_open_accumulation_window_is_refused(eng, monkeypatch):
    monkeypatch.setattr(eng, "_window_open", True)
    with pytest.raises(RuntimeError, match="accumulation window is open"):
        eng.train_window(_batches((2, 2)), TASK)


@pytest.mark.parametrize("task", ["cap%tva%tv", "qa%tva", "pt_caption%tva_mlm%tva"])
def test_a_task_without_contrastive_groups_is_refused(eng, task):
    """nothing spans the window: ValueError, not a silent plain accumulation"""
    with pytest.raises(ValueError, match="no contrastive groups"):
        eng.train_window(_batches((2, 2)), task)
    assert eng.global_step == 0 and not eng._window_open


def test_task_groups_parse_like_forward_pt_and_forward_ret(eng):
    m = eng.model
    assert m.task_groups(TASK) == (["tva"], ["tva", "tv", "ta"], ["tva", "tv", "ta"], m.contra_loss_ratio)
    assert m.task_groups("ret%tva%tv") == ([], [], ["tva", "tv"], 1.0)
    assert m.task_groups("cap%tva")[2] == [] and m.task_groups("qa%tv")[2] == []


def test_a_list_of_micro_batches_goes_through_the_window_step_only_when_asked(eng, monkeypatch):
    calls = []
    monkeypatch.setattr(eng, "train_window", lambda batches, task: calls.append((len(batches), task)) or {"contra_loss": 0.0})
    bs = _batches((2, 2))
    with pytest.raises(TypeError, match="contra_window"):
        eng.train_step(bs, TASK)
    monkeypatch.setattr(eng, "contra_window", True)
    assert eng.train_step(bs, TASK) == {"contra_loss": 0.0} and calls == [(2, TASK)]
    with pytest.raises(ValueError, match="accum_steps"):
        eng.train_step(bs, TASK, accum_steps=2)
    # the option spelling
    spec = synth.tiny_spec()
    model = VALOR({"dropout": 0.0}, spec=spec, dtype=torch.float32, device="cpu")
    o = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, betas=[0.9, 0.98], contra_window=True)
    assert TrainEngine(model, o, manage_gc=False).contra_window is True
    assert TrainEngine(model, o, manage_gc=False, contra_window=False).contra_window is False


def test_micro_batch_size_reads_tokens_then_inputs():
    b = _batches((3,))[0]
    assert E.micro_batch_size(b) == 3
    assert E.micro_batch_size({"video_pixels": torch.zeros(5, 1, 3, 8, 8)}) == 5
    with pytest.raises(ValueError):
        E.micro_batch_size({})


def test_bank_rows_are_the_micro_batches_in_order():
    """micro-batch m owns rows [m b, (m + 1) b) of every bank tensor, a modality the task does not use stays None, the bank's features are
    leaves that take a gradient and do not alias the passes' tensors' history, and a gradient slice goes back to the right micro-batch"""
    M, b = 3, 2
    g = torch.Generator().manual_seed(0)
    passes = [SimpleNamespace(feat_t=torch.randn(b, 5, 4, generator=g), feat_v=torch.randn(b, 2, 4, generator=g), feat_a=None,
                              tokens=torch.randint(0, 9, (b, 5), generator=g)) for _ in range(M)]
    bank = E.window_bank(passes)
    assert bank["feat_a"] is None
    assert bank["feat_t"].shape == (M * b, 5, 4) and bank["feat_v"].shape == (M * b, 2, 4) and bank["tokens"].shape == (M * b, 5)
    assert bank["feat_t"].is_leaf and bank["feat_t"].requires_grad and bank["feat_v"].requires_grad and not bank["tokens"].is_floating_point()
    for m in range(M):
        assert torch.equal(E.bank_slice(bank["feat_t"], m, b), passes[m].feat_t)
        assert torch.equal(E.bank_slice(bank["feat_v"], m, b), passes[m].feat_v)
        assert torch.equal(E.bank_slice(bank["tokens"], m, b), passes[m].tokens)
    # a loss that weights micro-batch m's rows by m + 1: its gradient slices are those weights
    w = torch.arange(1, M + 1, dtype=torch.float32).repeat_interleave(b)[:, None, None]
    (bank["feat_t"] * w).sum().backward()
    for m in range(M):
        assert torch.equal(E.bank_slice(bank["feat_t"].grad, m, b), torch.full((b, 5, 4), float(m + 1)))
    # coarse features are 2-D: same row rule
    flat = E.window_bank([SimpleNamespace(feat_t=torch.full((b, 4), float(i)), feat_v=None, feat_a=None, tokens=None) for i in range(M)])
    assert flat["tokens"] is None and torch.equal(E.bank_slice(flat["feat_t"], 2, b), torch.full((b, 4), 2.0))
    with pytest.raises(ValueError, match="some micro-batches only"):
        E.window_bank([SimpleNamespace(feat_t=torch.zeros(b, 4), feat_v=None, feat_a=None, tokens=None),
                       SimpleNamespace(feat_t=None, feat_v=None, feat_a=None, tokens=None)])


def test_dropout_window_handle_host_mode():
    """window() / rewind() in host mode: the second pass over a micro-batch draws the windows the first one drew"""
    D = ops.DropoutState
    D.reset(9)
    D.draw(100)
    w0 = D.window()
    first = [D.draw(4096), D.draw_elems(17)]
    w1 = D.window()
    second = [D.draw(64)]
    tail = D.offset
    D.rewind(w0)
    assert [D.draw(4096), D.draw_elems(17)] == first and D.window() == w1
    D.rewind(w1)
    assert [D.draw(64)] == second and D.offset == tail
    assert D.base is None


def test_window_pass_checks_the_replay_and_jumps_past_the_other_windows():
    D = ops.DropoutState
    D.reset(3)
    # feature pass: remembers where its draws ended
    D.draw(1000)
    fp = WindowPass(features_only=True)
    ft = torch.zeros(2, 3, 4)
    fp.at_features(ft, None, ft, torch.ones(2, 3))
    assert fp.draws_end == D.offset == 251 and fp.feat_t is ft and fp.feat_a is ft and fp.feat_v is None
    # ... a later micro-batch's feature pass moved on; the training pass rewinds, draws the same, then jumps behind everything
    D.draw(1000)
    tail = D.offset
    D.rewind((0, 0))
    D.draw(1000)
    tp = WindowPass(features_only=False, draws_end=fp.draws_end, resume=tail)
    tp.at_features(ft, None, ft, None)
    assert D.offset == tail
    # a training pass that drew differently in front of the features is an error, not a silently different mask
    D.rewind((0, 0))
    D.draw(996)
    with pytest.raises(RuntimeError, match="the passes differ"):
        WindowPass(features_only=False, draws_end=fp.draws_end, resume=tail).at_features(ft, None, ft, None)
