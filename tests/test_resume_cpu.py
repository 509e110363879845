"""CPU: the host side of exact-resume checkpoints (valor_amd/checkpoint.py save_run / latest_step / resume_run, TrainEngine.state_dict /
load_state_dict and the state() / set_state() helpers of the RNG owners). Nothing here launches a kernel: the models are built on the
CPU (tables and arenas only) and the one train_step that runs uses a stand-in forward. The device side -- bit-identical continuation --
is tests/test_resume_gpu.py."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from valor_amd import checkpoint, decode, ops, synth
from valor_amd.engine import TrainEngine, host_rng_state, set_host_rng_state
from valor_amd.model.valor import VALOR, DeviceTokenMasker


@pytest.fixture(autouse=True)
def host_mode():
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)


def _engine(masker="host", dtype=torch.bfloat16, weight_seed=3, **opts):
    spec = synth.tiny_spec()
    model = VALOR({"dropout": 0.1, "token_masker": masker}, spec=spec, dtype=dtype, device="cpu")
    model.load_state_dict(synth.make_state_dict(spec, seed=weight_seed))
    o = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, betas=[0.9, 0.98], num_train_steps=100, warmup_ratio=0.1, **opts)
    return model, TrainEngine(model, o, manage_gc=False)


def test_dropout_state_round_trip_host_mode():
    D = ops.DropoutState
    D.reset(77)
    D.draw(1000); D.draw_elems(333)
    st = D.state()
    assert st == {"mode": "host", "seed": 77, "offset": 251 + 334, "base": 0}
    want = [D.draw(4096), D.draw_elems(17), D.draw(5)]
    D.reset(5)
    D.draw(99)
    D.set_state(st)
    assert [D.draw(4096), D.draw_elems(17), D.draw(5)] == want
    with pytest.raises(ValueError):
        D.set_state(dict(st, mode="eager"))
    # a device-mode state met in host mode is not applied and not dropped: it waits for the counter, and a step refuses to start meanwhile
    D.reset(5)
    D.set_state({"mode": "device", "seed": 9, "offset": 3, "base": 4 << 40})
    assert (D.seed, D.offset) == (5, 0)
    with pytest.raises(ValueError):
        D.check_restored()
    D.reset(5)
    D.check_restored()


def test_device_token_masker_round_trip():
    a = DeviceTokenMasker(103, 106, 1000, put=lambda t: t, seed=21)
    a.calls, a.offset = 7, 7 * 2 * 32
    a.philox_key(0)
    st = a.state()
    assert st == {"seed": 21, "calls": 7, "offset": 448} and all(type(v) is int for v in st.values())
    b = DeviceTokenMasker(103, 106, 1000, put=lambda t: t, seed=99)
    b.philox_key(0); b.philox_key(1)                        # keys cached under the other seed must not survive the restore
    b.set_state(st)
    assert (b.seed, b.calls, b.offset) == (a.seed, a.calls, a.offset)
    assert b.philox_key(0) == a.philox_key(0) and b.philox_key(1) == a.philox_key(1) and a.philox_key(0) != a.philox_key(1)
    assert b.philox_key(0) != DeviceTokenMasker(103, 106, 1000, put=lambda t: t, seed=99).philox_key(0)


def test_sample_stream_round_trip():
    a = decode.SampleStream(seed=7)
    a.begin_call(); a.take(3, 1000); a.begin_call(); a.take(3, 1000)
    st = a.state()
    assert st == {"seed": 7, "calls": 2, "offset": 750}
    b = decode.SampleStream(seed=1)
    b.set_state(st)
    assert b.take(6, 30522) == a.take(6, 30522)             # the call under way: same key, same window
    b.begin_call(); a.begin_call()
    assert b.take(2, 999) == a.take(2, 999) and b.key == a.key and b.calls == 3
    # the model-level helpers: no stream yet <-> None
    model, eng = _engine()
    assert decode.sampler_state(model) is None
    decode.sampler_of(model).begin_call()
    assert decode.sampler_state(model)["calls"] == 1
    decode.set_sampler_state(model, None)
    assert decode.sampler_state(model) is None
    decode.set_sampler_state(model, st)
    assert decode.sampler_of(model).state() == st
    eng.close()


def test_host_rng_state_round_trip():
    random.seed(3); np.random.seed(4); torch.manual_seed(5)
    random.gauss(0, 1); np.random.standard_normal()         # both generators now hold a cached second normal: part of the state
    st = host_rng_state()
    want = (random.random(), random.gauss(0, 1), np.random.random_sample(3).tolist(), np.random.standard_normal(), torch.rand(3))
    random.seed(30); np.random.seed(40); torch.manual_seed(50)
    set_host_rng_state(st)
    got = (random.random(), random.gauss(0, 1), np.random.random_sample(3).tolist(), np.random.standard_normal(), torch.rand(3))
    assert got[:4] == want[:4] and torch.equal(got[4], want[4])


def test_engine_file_loads_with_weights_only_and_round_trips(tmp_path):
    model, eng = _engine(masker="device")
    ops.DropoutState.reset(31)
    ops.DropoutState.draw(12345)
    model.device_masker.calls, model.device_masker.offset = 4, 256
    decode.sampler_of(model).begin_call().take(2, 1000)
    eng.global_step, eng._micro, eng._task = 12, 24, "pt_mlm%tva"
    random.seed(8); np.random.seed(9)
    handle = checkpoint.save_run(eng, str(tmp_path))
    assert handle.wait() == 12 and handle.done()
    files = checkpoint.run_files(str(tmp_path), 12)
    assert sorted(os.listdir(tmp_path / "ckpt")) == sorted(os.path.basename(f) for f in files.values())
    sd = torch.load(files["engine"], weights_only=True)
    assert sd["format"] == "valor_amd.engine/1" and sd["world_size"] == 1 and sd["rank"] == 0 and sd["global_step"] == 12
    assert sd["task"] == ["pt_mlm%tva"] and sd["dropout"] == {"mode": "host", "seed": 31, "offset": 3088, "base": 0}
    assert sd["device_masker"] == {"seed": 42, "calls": 4, "offset": 256} and sd["sampler"] == {"seed": 42, "calls": 1, "offset": 500}

    def plain(x):
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        if isinstance(x, list):
            return all(plain(v) for v in x)
        return isinstance(x, (torch.Tensor, int, float, str)) and not isinstance(x, bool)
    assert plain(sd)
    # the other two files are weights_only-loadable too; the model file carries the reference's keys
    msd = torch.load(files["model"], weights_only=True)
    assert set(msd) == {k for k, _, _ in synth.state_dict_layout(model.spec)}
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in msd.items())
    osd = torch.load(files["optimizer"], weights_only=True)
    assert torch.equal(osd["master"], eng.optimizer.master) and osd["names"] == list(model.arena.offsets)
    want = (random.random(), np.random.random_sample())
    # a fresh engine with everything different
    model2, eng2 = _engine(masker="device", weight_seed=4)
    ops.DropoutState.reset(1)
    random.seed(80); np.random.seed(90)
    assert checkpoint.resume_run(eng2, str(tmp_path)) == 12
    assert (eng2.global_step, eng2._micro, eng2._task) == (12, 24, "pt_mlm%tva")
    assert ops.DropoutState.state() == sd["dropout"]
    assert model2.device_masker.state() == sd["device_masker"] and decode.sampler_state(model2) == sd["sampler"]
    assert (random.random(), np.random.random_sample()) == want
    assert torch.equal(model2.arena.flat, model.arena.flat) and torch.equal(eng2.optimizer.master, eng.optimizer.master)
    eng.close(); eng2.close()


def test_latest_step_ignores_incomplete_steps_and_temporary_files(tmp_path):
    assert checkpoint.latest_step(str(tmp_path)) is None
    d = tmp_path / "ckpt"
    d.mkdir()
    assert checkpoint.latest_step(str(tmp_path)) is None
    for name in ("model_step_5.pt", "optimizer_step_5.pt", "engine_step_5.rank0.pt",
                 "model_step_3.pt", "optimizer_step_3.pt", "engine_step_3.rank0.pt",
                 "model_step_9.pt", "engine_step_9.rank0.pt",                               # optimizer file missing
                 "model_step_11.pt", "optimizer_step_11.pt", "engine_step_11.rank1.pt",     # another rank's engine file only
                 "tmp.4242.model_step_20.pt", "tmp.4242.optimizer_step_20.pt", "tmp.4242.engine_step_20.rank0.pt",
                 "model_step_20.pt", "optimizer_step_20.pt",                                # killed while the engine file was being written
                 "model_step_30.pt.part", "best_ret.pt", "notes.txt"):
        (d / name).write_bytes(b"")
    assert checkpoint.latest_step(str(tmp_path)) == 5
    assert checkpoint.latest_step(str(tmp_path), rank=1) == 11
    assert checkpoint.latest_step(str(tmp_path), need_engine=False) == 20


@pytest.mark.parametrize("remove", [True, False])
def test_remove_before_ckpt_leaves_the_newest_step(tmp_path, remove):
    model, eng = _engine(remove_before_ckpt=remove)
    (tmp_path / "ckpt").mkdir()
    (tmp_path / "ckpt" / "engine_step_1.rank3.pt").write_bytes(b"")        # another rank's file is that rank's to remove
    for step in (1, 2, 3):
        eng.global_step = step
        checkpoint.save_run(eng, str(tmp_path))
    left = sorted(os.listdir(tmp_path / "ckpt"))
    newest = ["engine_step_1.rank3.pt", "engine_step_3.rank0.pt", "model_step_3.pt", "optimizer_step_3.pt"]
    if remove:
        assert left == newest
    else:
        assert len(left) == 10 and set(newest) <= set(left)
    assert checkpoint.latest_step(str(tmp_path)) == 3
    eng.close()


def test_default_is_to_remove_older_steps(tmp_path):
    model, eng = _engine()
    for step in (4, 8):
        eng.global_step = step
        checkpoint.save_run(eng, str(tmp_path))
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["engine_step_8.rank0.pt", "model_step_8.pt", "optimizer_step_8.pt"]
    eng.close()


def test_state_dict_inside_an_accumulation_window_raises(tmp_path):
    """the first micro-step of a window of two returns without an optimizer step: no checkpoint there (a stand-in forward: the flag is
    train_step's, not the model's)"""
    model, eng = _engine(dtype=torch.float32)
    model.forward = lambda batch, task, compute_loss=True: {"loss": (model.P["contra_temp"].float() ** 2).sum()}
    eng.state_dict()
    eng.train_step({}, "pt_mlm%tva", accum_steps=2)
    assert eng.global_step == 0
    with pytest.raises(RuntimeError, match="accumulation window"):
        eng.state_dict()
    with pytest.raises(RuntimeError, match="accumulation window"):
        checkpoint.save_run(eng, str(tmp_path))
    assert not os.path.isdir(tmp_path / "ckpt") or os.listdir(tmp_path / "ckpt") == []
    eng.close()


def test_world_size_and_masker_mode_mismatch_raise():
    model, eng = _engine(masker="host")
    sd = eng.state_dict()
    eng.load_state_dict(sd)
    with pytest.raises(ValueError, match="world size"):
        eng.load_state_dict(dict(sd, world_size=2))
    with pytest.raises(ValueError, match="format"):
        eng.load_state_dict(dict(sd, format="something/0"))
    model_d, eng_d = _engine(masker="device")
    with pytest.raises(ValueError, match="token_masker"):
        eng_d.load_state_dict(sd)
    with pytest.raises(ValueError, match="token_masker"):
        eng.load_state_dict(eng_d.state_dict())
    # nothing was changed by the refused loads
    eng.global_step = 5
    with pytest.raises(ValueError):
        eng.load_state_dict(dict(sd, world_size=2))
    assert eng.global_step == 5
    eng.close(); eng_d.close()


def test_resume_without_an_engine_file_is_explicit(tmp_path):
    """a checkpoint the reference wrote (model + torch-Optimizer layout, no engine file): refused by default, continued with fresh RNG
    state on request"""
    model, eng = _engine()
    eng.optimizer.steps = {n: 3 for n in model.arena.offsets}
    eng.optimizer.exp_avg.normal_(generator=torch.Generator().manual_seed(1))
    (tmp_path / "ckpt").mkdir()
    torch.save({k: v.clone() for k, v in model.state_dict().items()}, tmp_path / "ckpt" / "model_step_7.pt")
    torch.save(eng.optimizer.reference_state_dict(), tmp_path / "ckpt" / "optimizer_step_7.pt")
    model2, eng2 = _engine(weight_seed=4)
    with pytest.raises(FileNotFoundError, match="allow_inexact"):
        checkpoint.resume_run(eng2, str(tmp_path))
    with pytest.raises(FileNotFoundError, match="allow_inexact"):
        checkpoint.resume_run(eng2, str(tmp_path), step=7)
    assert eng2.global_step == 0 and not torch.equal(model2.arena.flat, model.arena.flat)
    assert checkpoint.resume_run(eng2, str(tmp_path), allow_inexact=True) == 7
    assert eng2.global_step == 7 and torch.equal(model2.arena.flat, model.arena.flat)
    for o, n, _ in model.arena.offsets.values():
        assert torch.equal(eng2.optimizer.exp_avg[o:o + n], eng.optimizer.exp_avg[o:o + n])
    assert set(eng2.optimizer.steps.values()) == {3}
    eng.close(); eng2.close()
