"""Exact resume on the device (train_utils.py:174-192,226-228 + utils/save.py:38-64 of the reference, which restores weights and
optimizer and nothing else): save_run in the middle of a run -> a FRESH model (other weights), optimizer and TrainEngine in a process
state that was deliberately scrambled (other dropout seed, reseeded `random` / numpy) -> resume_run -> the next steps equal the
uninterrupted run's TO THE BIT: every loss, the parameter arena, fp32 masters, both moments, the per-tensor step counts, every lr.
All comparisons are torch.equal / ==; there is no tolerance in this file except the one the golden fixture of the last test brings.

The saves sit after the fourth step, i.e. after the graph capture inside the third: the resumed engine runs eagerly where the
uninterrupted one replays, so every graphs-on case also checks replay == eager on restored state."""
import gc
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(autouse=True)
def rng_modes(dev):
    from valor_amd import ops
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    gc.collect()            # the models of this test and their (released) graph segments go now, not in the middle of a later test's capture


def _opts(**kw):
    return SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-4, clip_lr_text=1e-4, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0, **kw)


class Cfg:
    """one run configuration; hashable by its fields so the uninterrupted reference run is computed once per configuration"""

    def __init__(self, graphs=True, masker="host", swin=False, scst=False, accum=1):
        self.graphs, self.masker, self.swin, self.scst, self.accum = graphs, masker, swin, scst, accum

    @property
    def key(self):
        return (self.graphs, self.masker, self.swin, self.scst, self.accum)

    @property
    def task(self):
        return "cap%tv" if self.scst else TASK

    def batch(self, dev, i):
        from valor_amd import synth
        spec = self.spec()
        b = synth.make_batch(spec, batch=3 if self.scst else 2, frames=2, audio_slices=1, txt_len=16 if self.scst else 32, seed=10 + i)
        b["ids"] = [f"clip{j}" for j in range(3 if self.scst else 2)]
        b["video_pixels"] = b["video_pixels"].to(dev)
        b["audio_spectrograms"] = b["audio_spectrograms"].to(dev)
        return b

    def spec(self):
        from valor_amd import synth
        return synth.tiny_swin_spec() if self.swin else synth.tiny_spec()

    def build(self, dev, weight_seed, graphs=None):
        """model + engine (graphs: override, for the restore-order test that switches them on by hand)"""
        from valor_amd import scst, synth
        from valor_amd.engine import TrainEngine
        from valor_amd.model.valor import VALOR
        spec = self.spec()
        sd = synth.make_state_dict(spec, seed=weight_seed, w_std=0.05)
        mo = {"dropout": 0.1, "drop_path_rate": 0.2 if self.swin else 0.0, "token_masker": self.masker, "seed": 7}
        if self.scst:
            mo.update(max_generation_len=8, scst_finetuning=True)
        model = VALOR(mo, spec=spec, dtype=torch.float32 if self.scst else torch.bfloat16, device=dev)      # scst: as tests/test_scst_gpu.py
        model.load_state_dict(sd, strict=True)
        if self.scst:
            rng = np.random.default_rng(0)
            model.scorer = scst.CaptionScorer({f"clip{i}": [rng.integers(1000, 1040, size=6).tolist() for _ in range(3)] for i in range(3)})
        eng = TrainEngine(model, _opts(), manage_gc=False, graphs=self.graphs if graphs is None else graphs)
        eng.optimizer.init_master_from(sd)
        return model, eng


def _seed_run(seed):
    from valor_amd import ops
    ops.DropoutState.reset(seed)
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    torch.manual_seed(seed + 3)


def _snapshot(eng, out):
    opt = eng.optimizer
    return {"losses": {k: v.detach().clone() for k, v in out.items()}, "flat": eng.model.arena.flat.detach().clone(), "master": opt.master.clone(),
            "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(), "steps": opt.steps,
            "lr": [g["lr"] for g in opt.param_groups], "global_step": eng.global_step}


def _same(got, want, what):
    assert got["losses"].keys() == want["losses"].keys(), what
    for k in want["losses"]:
        assert torch.equal(got["losses"][k], want["losses"][k]), (what, k, float(got["losses"][k]), float(want["losses"][k]))
    for k in ("flat", "master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
    assert got["steps"] == want["steps"], what
    assert got["lr"] == want["lr"] and got["global_step"] == want["global_step"], what


def _steps(cfg, dev, eng, first, n, poison=None):
    """optimizer steps first+1 .. first+n (accum micro-steps each), a snapshot after every one"""
    snaps = []
    for s in range(first, first + n):
        for m in range(cfg.accum):
            if poison is not None and s == poison:
                arena = eng.model.arena
                o, cnt, _ = arena.offsets[next(nm for nm in arena.offsets if "word_embeddings" in nm)]
                arena.grad[o + cnt // 2] = float("nan")
            out = eng.train_step(cfg.batch(dev, s * cfg.accum + m), cfg.task, accum_steps=cfg.accum)
        snaps.append(_snapshot(eng, out))
    return snaps


def _teardown(model, eng):
    from valor_amd import decode
    torch.cuda.synchronize()
    model.enable_graphs(False)
    decode.release_sessions(model)
    eng.close()


_REFERENCE = {}


def _uninterrupted(cfg, dev, total=6, poison=None):
    key = cfg.key + (total, poison)
    if key not in _REFERENCE:
        _seed_run(77)
        model, eng = cfg.build(dev, weight_seed=3)
        _REFERENCE[key] = _steps(cfg, dev, eng, 0, total, poison)
        if cfg.graphs and not cfg.scst:
            assert model._graph_segs and all(len(s.captured) >= 1 for s in model._graph_segs.values())         # it did replay
        _teardown(model, eng)
    return _REFERENCE[key]


def _scramble():
    """a process state in which only the load can make the runs agree"""
    _seed_run(4000)


def _saved_run(cfg, dev, out_dir, upto=4, poison=None, blocking=True):
    from valor_amd import checkpoint
    _seed_run(77)
    model, eng = cfg.build(dev, weight_seed=3)
    snaps = _steps(cfg, dev, eng, 0, upto, poison)
    handle = checkpoint.save_run(eng, out_dir, blocking=blocking)
    return model, eng, snaps, handle


CASES = [pytest.param(Cfg(graphs=g, masker=m, swin=s), id=f"{'graphs' if g else 'eager'}-{m}-{'swin' if s else 'clip'}")
         for g in (True, False) for m in ("host", "device") for s in (False, True)]
CASES.append(pytest.param(Cfg(graphs=True, scst=True), id="scst-cap_tv"))


@pytest.mark.parametrize("cfg", CASES)
def test_resumed_run_continues_bit_identically(dev, tmp_path, cfg):
    """six steps against four steps + save_run + a fresh, differently initialised everything + resume_run + two steps"""
    from valor_amd import checkpoint, ops
    want = _uninterrupted(cfg, dev)
    model, eng, snaps, _ = _saved_run(cfg, dev, str(tmp_path))
    for i, s in enumerate(snaps):
        _same(s, want[i], f"before the save, step {i + 1}")          # the run is reproducible at all
    assert ops.DropoutState.state()["mode"] == ("device" if cfg.graphs else "host")
    _teardown(model, eng)
    del model, eng
    _scramble()
    model, eng = cfg.build(dev, weight_seed=11)
    assert not torch.equal(model.arena.flat, want[3]["flat"])
    assert checkpoint.resume_run(eng, str(tmp_path)) == 4 == checkpoint.latest_step(str(tmp_path))
    got = _steps(cfg, dev, eng, 4, 2)
    _same(got[0], want[4], "step 5")
    _same(got[1], want[5], "step 6")
    assert not torch.equal(want[4]["flat"], want[5]["flat"]) and want[4]["losses"].keys() and \
        any(not torch.equal(want[4]["losses"][k], want[5]["losses"][k]) for k in want[4]["losses"])            # the steps do differ
    _teardown(model, eng)


@pytest.mark.parametrize("engine_first", [True, False], ids=["engine_before_enable_graphs", "engine_after_enable_graphs"])
@pytest.mark.parametrize("model_first", [True, False], ids=["model_then_optimizer", "optimizer_then_model"])
def test_restore_order_is_free(dev, tmp_path, engine_first, model_first):
    """the three loads by hand in every order: the engine state before model.enable_graphs() (the dropout counter does not exist yet;
    enable_device_base zeroes a new one) and after; model then optimizer and optimizer then model (the fp32 masters' low bits)"""
    from valor_amd import checkpoint
    cfg = Cfg(graphs=True)
    want = _uninterrupted(cfg, dev)
    model, eng, _, _ = _saved_run(cfg, dev, str(tmp_path))
    _teardown(model, eng)
    del model, eng
    _scramble()
    files = checkpoint.run_files(str(tmp_path), 4)
    esd, msd, osd = (torch.load(files[k], map_location="cpu", weights_only=True) for k in ("engine", "model", "optimizer"))
    model, eng = cfg.build(dev, weight_seed=11, graphs=False)

    def weights():
        if model_first:
            model.load_state_dict(msd); eng.optimizer.load_state_dict(osd)
        else:
            eng.optimizer.load_state_dict(osd); model.load_state_dict(msd)
    if engine_first:
        eng.load_state_dict(esd)
        weights()
        model.enable_graphs()
    else:
        model.enable_graphs()
        weights()
        eng.load_state_dict(esd)
    got = _steps(cfg, dev, eng, 4, 2)
    _same(got[0], want[4], "step 5")
    _same(got[1], want[5], "step 6")
    _teardown(model, eng)


@pytest.mark.parametrize("left_out", ["dropout", "host_rng", "device_masker", "global_step"])
def test_every_restored_piece_is_needed(dev, tmp_path, left_out):
    """the control of the tests above: the same resume with ONE piece of the engine state left as the scrambled process had it does not
    continue the run (so the agreement above comes from the restore, not from runs that agree anyway). dropout: seed / offset / device
    counter; host_rng: Python `random` drives the host masker; device_masker: its call index and counter window; global_step: the lr."""
    from valor_amd import checkpoint, ops
    from valor_amd.engine import host_rng_state
    cfg = Cfg(graphs=True, masker="device" if left_out == "device_masker" else "host")
    want = _uninterrupted(cfg, dev)
    model, eng, _, _ = _saved_run(cfg, dev, str(tmp_path))
    _teardown(model, eng)
    del model, eng
    _scramble()
    files = checkpoint.run_files(str(tmp_path), 4)
    esd, msd, osd = (torch.load(files[k], map_location="cpu", weights_only=True) for k in ("engine", "model", "optimizer"))
    model, eng = cfg.build(dev, weight_seed=11)
    esd[left_out] = {"dropout": ops.DropoutState.state, "host_rng": host_rng_state, "device_masker": lambda: model.device_masker.state(),
                     "global_step": lambda: 0}[left_out]()
    eng.load_state_dict(esd)
    model.load_state_dict(msd)
    eng.optimizer.load_state_dict(osd)
    assert torch.equal(model.arena.flat, want[3]["flat"]) and torch.equal(eng.optimizer.master, want[3]["master"])
    got = _steps(cfg, dev, eng, 4, 1)[0]
    if left_out == "global_step":
        assert got["lr"] != want[4]["lr"]
    else:
        assert any(not torch.equal(got["losses"][k], want[4]["losses"][k]) for k in want[4]["losses"])
    assert not torch.equal(got["flat"], want[4]["flat"])
    _teardown(model, eng)


def test_dropout_mode_mismatch_is_refused(dev):
    """the mode follows graphs on / off and changes the draws: a state saved with graphs on does not continue a graphs-off engine (refused
    when the step starts: until then enable_graphs() may still come) and the other way round (refused at the load)"""
    cfg = Cfg(graphs=True)
    model, eng = cfg.build(dev, weight_seed=3)
    on = eng.state_dict()
    _teardown(model, eng)
    model, eng = cfg.build(dev, weight_seed=3, graphs=False)
    off = eng.state_dict()
    assert (on["dropout"]["mode"], off["dropout"]["mode"]) == ("device", "host")
    eng.load_state_dict(on)
    with pytest.raises(ValueError, match="device mode"):
        eng.train_step(cfg.batch(dev, 0), cfg.task)
    from valor_amd import ops
    ops.DropoutState.reset(1234)
    model.enable_graphs()
    with pytest.raises(ValueError, match="host mode"):
        eng.load_state_dict(off)
    _teardown(model, eng)


def test_accumulation_window(dev, tmp_path):
    """accum_steps = 2: a save after a closed window continues identically; a save after the window's first micro-step raises"""
    from valor_amd import checkpoint
    cfg = Cfg(graphs=True, accum=2)
    want = _uninterrupted(cfg, dev, total=3)
    model, eng, snaps, _ = _saved_run(cfg, dev, str(tmp_path), upto=2)
    _same(snaps[1], want[1], "window 2")
    eng.train_step(cfg.batch(dev, 4), cfg.task, accum_steps=2)               # window 3 opens
    with pytest.raises(RuntimeError, match="accumulation window"):
        checkpoint.save_run(eng, str(tmp_path))
    with pytest.raises(RuntimeError, match="accumulation window"):
        eng.state_dict()
    assert checkpoint.latest_step(str(tmp_path)) == 2
    _teardown(model, eng)
    del model, eng
    _scramble()
    model, eng = cfg.build(dev, weight_seed=11)
    assert checkpoint.resume_run(eng, str(tmp_path)) == 2
    got = _steps(cfg, dev, eng, 2, 1)
    _same(got[0], want[2], "window 3")
    _teardown(model, eng)


def test_nonblocking_save_is_a_snapshot_of_its_step(dev, tmp_path):
    """save_run(blocking=False) after step 3, steps 4 and 5 issued at once, then wait(): the files hold the state right after step 3 (not
    the state two optimizer steps later), the steps issued beside the save are the uninterrupted run's, and a resume from the files
    reproduces steps 4 and 5. A second non-blocking save reuses the buffers; engine.close() waits for it."""
    from valor_amd import checkpoint
    cfg = Cfg(graphs=True)
    want = _uninterrupted(cfg, dev)
    _seed_run(77)
    model, eng = cfg.build(dev, weight_seed=3)
    eng.opts.remove_before_ckpt = False                  # both saves of this test stay on disk
    at3 = _steps(cfg, dev, eng, 0, 3)[-1]
    handle = checkpoint.save_run(eng, str(tmp_path), blocking=False)
    later = _steps(cfg, dev, eng, 3, 2)
    assert handle.wait() == 3 and handle.done()
    _same(later[0], want[3], "step 4 beside the save")
    _same(later[1], want[4], "step 5 beside the save")
    files = checkpoint.run_files(str(tmp_path), 3)
    msd, osd = (torch.load(files[k], map_location=dev, weights_only=True) for k in ("model", "optimizer"))
    want_model, now_model = model.state_dict(flat=at3["flat"]), model.state_dict()
    assert set(msd) == set(want_model)
    assert all(torch.equal(msd[k], want_model[k]) for k in msd)
    assert any(not torch.equal(msd[k], now_model[k]) for k in msd if msd[k].is_floating_point())
    assert torch.equal(osd["master"], at3["master"]) and not torch.equal(osd["master"], eng.optimizer.master)
    names, offsets = osd["names"], model.arena.offsets
    assert len(osd["state"]) > 50
    for i, st in osd["state"].items():
        o, n, _ = offsets[names[i]]
        assert st["step"] == at3["steps"][names[i]]
        assert torch.equal(st["exp_avg"].reshape(-1), at3["exp_avg"][o:o + n]) and torch.equal(st["exp_avg_sq"].reshape(-1), at3["exp_avg_sq"][o:o + n])
    assert [g["lr"] for g in osd["param_groups"]] == at3["lr"] != later[1]["lr"]
    # a second one: same buffers, waits for the first; close() waits for it
    saver = eng._saver
    ptrs = {k: t.data_ptr() for k, t in saver.host.items()}
    h2 = checkpoint.save_run(eng, str(tmp_path), blocking=False)
    eng.close()
    assert h2.done() and h2.wait() == 5 and eng._saver is saver and ptrs == {k: t.data_ptr() for k, t in saver.host.items()}
    assert sorted(os.listdir(tmp_path / "ckpt")) == sorted(f"{k}_step_{n}{r}.pt" for n in (3, 5) for k, r in (("engine", ".rank0"), ("model", ""), ("optimizer", "")))
    assert torch.equal(torch.load(checkpoint.run_files(str(tmp_path), 5)["optimizer"], map_location=dev, weights_only=True)["master"], later[1]["master"])
    _teardown(model, eng)
    del model, eng
    _scramble()
    model, eng = cfg.build(dev, weight_seed=11)
    assert checkpoint.resume_run(eng, str(tmp_path), step=3) == 3
    got = _steps(cfg, dev, eng, 3, 2)
    _same(got[0], later[0], "step 4")
    _same(got[1], later[1], "step 5")
    _teardown(model, eng)


def test_skipped_step_counts_survive(dev, tmp_path):
    """step 3 meets a NaN gradient (planted in the arena the way tests/test_optimizer_gpu.py plants it): the update is skipped on the
    device, the per-tensor counts stay at 2 while global_step -- and the LR schedule -- move to 3. Saved right after it: the resumed
    counts, and the next update's bias corrections with them, are the uninterrupted run's."""
    import math
    from valor_amd import checkpoint
    cfg = Cfg(graphs=True)
    want = _uninterrupted(cfg, dev, total=5, poison=2)
    assert max(want[2]["steps"].values()) == 2 and want[2]["global_step"] == 3 and torch.equal(want[2]["master"], want[1]["master"])
    assert max(want[3]["steps"].values()) == 3 and not torch.equal(want[3]["master"], want[2]["master"])
    model, eng, snaps, _ = _saved_run(cfg, dev, str(tmp_path), upto=3, poison=2)
    assert not math.isfinite(float(eng.optimizer.total_norm))
    _same(snaps[2], want[2], "the skipped step")
    _teardown(model, eng)
    del model, eng
    _scramble()
    model, eng = cfg.build(dev, weight_seed=11)
    assert checkpoint.resume_run(eng, str(tmp_path)) == 3
    assert eng.optimizer.steps == want[2]["steps"]
    got = _steps(cfg, dev, eng, 3, 2)
    _same(got[0], want[3], "step 4")
    _same(got[1], want[4], "step 5")
    _teardown(model, eng)


# ---------------------------------------------------------------------------------------------- adapted checkpoints on the device
def test_adapted_checkpoint_gives_the_fixture_losses(dev):
    """A `model_step_N.pt` of a pretraining run through the reference's loading path (train_utils.py:120-171, restated by
    checkpoint.adapt_pretrained_checkpoint) and into the native model on the device, on ref_base_b2f16a2_q (16 frames, 2 audio slices:
    frame-embedding rows 0..15 / 0..1 are live). The file has DDP's `module.` prefix and, behind the pretraining sample counts, frame
    embedding rows the run never trained (here: garbage); the adaptation strips the prefix and extends the last trained row over them,
    and the CLIP positional embedding goes through the bilinear resize of a bare --checkpoint (train.py:28-44; same grid: the
    interpolation reproduces its input to 1e-6). The losses are the fixture's, in the band tests/test_model_gpu.py holds this
    fixture to in fp32 (1e-4 relative)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_model_gpu import _native, _recipe_tensors
    from valor_amd.checkpoint import adapt_pretrained_checkpoint, resize_clip_positional_embedding
    g = torch.load(os.path.join(GOLD, "ref_base_b2f16a2_q.pt"), weights_only=False)
    rc = g["recipe"]
    assert (rc["frames"], rc["audio_slices"]) == (16, 2)
    spec, sd, batch = _recipe_tensors(rc)
    gen = torch.Generator().manual_seed(5)
    ck = {"module." + k: v.clone() for k, v in sd.items()}
    ck["module.video_frame_embedding"][:, 16:] = torch.randn(ck["module.video_frame_embedding"][:, 16:].shape, generator=gen) * 50
    ck["module.audio_frame_embedding"][:, 2:] = torch.randn(ck["module.audio_frame_embedding"][:, 2:].shape, generator=gen) * 50
    hps = {"video_sample_num": 16, "audio_sample_num": 2, "video_resolution": spec.resolution, "video_encoder_type": "clip_vit_base_16",
           "txt_encoder_type": "clip_vit_base_16", "contra_type": "fine"}
    opts = {"dropout": 0.0, "drop_path_rate": 0.0, "video_resolution": spec.resolution, "video_encoder_type": "x", "contra_type": "coarse"}
    adapted = adapt_pretrained_checkpoint(ck, hps, opts)
    assert opts["video_encoder_type"] == "clip_vit_base_16" and opts["contra_type"] == "fine" and set(adapted) == set(sd)
    v, a = adapted["video_frame_embedding"], adapted["audio_frame_embedding"]
    assert torch.equal(v[:, :16], sd["video_frame_embedding"][:, :16]) and all(torch.equal(v[:, i], v[:, 15]) for i in range(16, 32))
    assert torch.equal(a[:, :2], sd["audio_frame_embedding"][:, :2]) and all(torch.equal(a[:, i], a[:, 1]) for i in range(2, 32))
    resize_clip_positional_embedding(adapted, spec.resolution)
    pe = adapted["clip_model.visual.positional_embedding"]
    assert pe.shape == sd["clip_model.visual.positional_embedding"].shape and torch.allclose(pe, sd["clip_model.visual.positional_embedding"], atol=1e-6)
    model = _native(spec, adapted, torch.float32, dev)
    random.seed(rc["masker_seed"])
    with torch.no_grad():
        out = model(batch, task=rc["task"], compute_loss=True)
    for k, ref in g["steps"][0]["losses"].items():
        assert abs(float(out[k]) - ref) <= 1e-4 * abs(ref), (k, float(out[k]), ref)


def test_adapted_checkpoint_with_live_extension_matches_the_oracle(dev):
    """the adaptation where it changes what the step computes: a run pretrained with ONE frame / ONE audio slice at half the
    resolution, continued at two frames and the full resolution -- frame-embedding row 1 is the extended row 0, the CLIP positional
    embedding a 2 x 2 grid resized to 4 x 4. The adapted weights give the CPU oracle's losses on the device (fp32, 1e-4 relative: the
    band of tests/test_model_gpu.py::test_tiny_fp32_matches_oracle, the same spec and batch geometry)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import valor_oracle as VO
    from test_model_gpu import _native
    from valor_amd import synth
    from valor_amd.checkpoint import adapt_pretrained_checkpoint
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    gen = torch.Generator().manual_seed(6)
    ck = {k: v.clone() for k, v in sd.items()}
    ck["clip_model.visual.positional_embedding"] = torch.randn((2 * 2 + 1, spec.vis_width), generator=gen) * 0.05
    hps = {"video_sample_num": 1, "audio_sample_num": 1, "video_resolution": spec.resolution // 2}
    opts = {"dropout": 0.0, "drop_path_rate": 0.0, "video_resolution": spec.resolution, "video_encoder_type": "clip_vit_base_16"}
    adapted = adapt_pretrained_checkpoint(ck, hps, opts)
    assert adapted["clip_model.visual.positional_embedding"].shape == sd["clip_model.visual.positional_embedding"].shape
    assert torch.equal(adapted["video_frame_embedding"][:, 1], sd["video_frame_embedding"][:, 0])
    assert not torch.equal(adapted["video_frame_embedding"][:, 1], sd["video_frame_embedding"][:, 1])
    batch = synth.make_batch(spec, batch=4, frames=2, audio_slices=2, txt_len=32, seed=4)
    orc = VO.Oracle(spec, VO.trainable_copy(adapted), vocab_tokens=synth.synthetic_vocab(spec.vocab))
    model = _native(spec, adapted, torch.float32, dev)
    with torch.no_grad():
        random.seed(11); o_out = orc.forward_pt(batch, TASK, compute_loss=True)
        random.seed(11); n_out = model(batch, task=TASK, compute_loss=True)
        random.seed(11); plain = _native(spec, sd, torch.float32, dev)(batch, task=TASK, compute_loss=True)
    for k in ("contra_loss", "caption_loss", "mlm_loss"):
        a, b = float(o_out[k]), float(n_out[k])
        assert abs(a - b) <= 1e-4 * abs(a), (k, a, b)
    assert any(abs(float(plain[k]) - float(n_out[k])) > 1e-4 * abs(float(n_out[k])) for k in n_out)      # the adaptation is live in these losses
