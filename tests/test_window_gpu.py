"""The window step on the GPU (TrainEngine.train_window): M micro-batches, ONE contrastive evaluation over all N = M * b rows, one
optimizer step -- what the reference computes at world size M with micro-batch m as rank m (utils/distributed.py:38-93: every rank
evaluates the contrastive loss on the gathered features and back-propagates its own slice, DDP averages the gradients).

Expectations come from the CPU oracle with the reference's gather semantics restated through its `gather=` closures, exactly as
tests/test_dp_model_gpu.py::test_ranks_match_the_reference_semantics builds them for real ranks (shapes, seeds and tolerances are that
test's: tiny_spec, b = 2, 2 frames, 1 audio slice, 32 tokens; host masker seeded 100 + m for micro-batch m; losses to 1e-4 relative,
gradients to 2e-3 in relative norm per parameter):
  * contra_loss is the single-process loss on the full N-row batch; caption / mlm losses are the mean of the ranks' own;
  * the arena's gradient in front of the optimizer step is the mean over ranks of the oracle's per-rank gradients;
  * a parameter that only feeds the contrastive loss below the gather gets 1/M of the full-batch gradient, one applied to the
    gathered features (fine-weight heads, temperature, va_fusion) the full gradient.
Then: M = 1 is train_step to the bit; the feature pass and the training pass of a micro-batch produce bit-identical features under
dropout (host and device mode of the dropout state, graphs on and off, bf16 and fp32) and the host masker is consumed exactly as by M
plain steps; the contrastive kernels run once per group per window; and the result is NOT plain accumulation's."""
import dataclasses
import functools
import gc
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
B_LOCAL, FRAMES, SLICES = 2, 2, 1


@pytest.fixture(autouse=True)
def rng_modes(dev):
    from valor_amd import ops
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    gc.collect()


def _spec(variant):
    from valor_amd import synth
    if variant == "swin":
        return synth.tiny_swin_spec()
    if variant == "coarse":
        return dataclasses.replace(synth.tiny_spec(), contra_type="coarse")
    return synth.tiny_spec()


@functools.lru_cache(maxsize=None)
def _setup(variant, M):
    from valor_amd import synth
    spec = _spec(variant)
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    full = synth.make_batch(spec, batch=M * B_LOCAL, frames=FRAMES, audio_slices=SLICES, txt_len=32, seed=4)
    return spec, sd, full


def _part(full, m):
    sl = slice(m * B_LOCAL, (m + 1) * B_LOCAL)
    return {"ids": full["ids"][sl], "video_pixels": full["video_pixels"][sl], "audio_spectrograms": full["audio_spectrograms"][sl],
            "txt_tokens": {k: v[sl] for k, v in full["txt_tokens"].items()}}


def _opts(**kw):
    return SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-3, clip_lr_text=1e-3, new_lr=0.0, decoder_lr=-1,
                           betas=[0.9, 0.98], warmup_ratio=0.1, num_train_steps=10, scheduler="warmup_linear", grad_norm=5.0,
                           alloc_headroom_mb=0, **kw)


def _engine(spec, sd, dev, dtype=torch.float32, dropout=0.0, graphs=False, drop_path=0.0):
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    model = VALOR({"dropout": dropout, "drop_path_rate": drop_path}, spec=spec, dtype=dtype, device=dev)
    model.load_state_dict(sd, strict=True)
    eng = TrainEngine(model, _opts(), manage_gc=False, graphs=graphs)
    if dtype != torch.float32:
        eng.optimizer.init_master_from(sd)
    return model, eng


def _teardown(model, eng):
    torch.cuda.synchronize()
    model.enable_graphs(False)
    eng.close()


def _contra_only(task):
    return task if task.startswith("ret") else "pt_" + next(p for p in task.split("_") if "contra" in p)


@functools.lru_cache(maxsize=None)
def _expect(variant, M, task):
    """the oracle at world M, rank m = micro-batch m (computed once per configuration and shared): per-rank losses and gradients with the
    gather closures of tests/test_dp_model_gpu.py, and the single-process contrastive loss / gradients on the full batch"""
    import valor_oracle as VO
    from valor_amd import synth
    spec, sd, full = _setup(variant, M)
    vocab = synth.synthetic_vocab(spec.vocab)
    only = _contra_only(task)
    feats = []
    with torch.no_grad():
        for r in range(M):
            ev = VO.Oracle(spec, sd, vocab_tokens=vocab).forward(_part(full, r), only, compute_loss=False)
            feats.append({k: ev[k] for k in ("feat_t", "feat_v", "feat_a", "txt_tokens")})
    order = [k for k in ("feat_t", "feat_v", "feat_a") if feats[0][k] is not None]      # the order the oracle gathers in
    want_grads, want_losses = [], []
    for r in range(M):
        sd_r = VO.trainable_copy(sd)
        orc = VO.Oracle(spec, sd_r, vocab_tokens=vocab)
        calls = []

        def gather_feat(f, r=r, calls=calls):
            key = order[len(calls)]
            calls.append(key)
            parts = [feats[q][key] for q in range(M)]
            assert parts[r].shape == f.shape
            parts[r] = f                                             # the local slice carries the gradient (utils/distributed.py:62-72)
            return torch.cat(parts, dim=0)

        def gather_tok(t, r=r):
            return torch.cat([feats[q]["txt_tokens"] for q in range(M)], dim=0)

        random.seed(100 + r)
        out = orc.forward(_part(full, r), task, compute_loss=True, gather=(gather_feat, gather_tok))
        sum(out.values()).backward()
        assert calls == order
        want_losses.append({k: float(v.detach()) for k, v in out.items()})
        want_grads.append({k: (p.grad.clone() if p.grad is not None else None) for k, p in sd_r.items()
                           if p.is_floating_point() and not VO.is_alias_key(k)})
    sd_f = VO.trainable_copy(sd)
    lf = VO.Oracle(spec, sd_f, vocab_tokens=vocab).forward(full, only, compute_loss=True)["contra_loss"]
    lf.backward()
    full_grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in sd_f.items() if p.is_floating_point()}
    return want_losses, want_grads, float(lf.detach()), full_grads


def _seed_masker_per_micro_batch(model, batches, base):
    """the host masker of micro-batch m's training pass starts from random.seed(base + m), as rank m's does in test_dp_model_gpu.py"""
    orig = model.forward
    ids = [id(b) for b in batches]

    def forward(batch, task, compute_loss=True, window=None):
        if window is not None and not window.features_only:
            random.seed(base + ids.index(id(batch)))
        return orig(batch, task, compute_loss=compute_loss, window=window)
    model.forward = forward


def _grads_before_the_step(model, eng):
    """reference-keyed copies of the arena's gradients as the optimizer step of the next window finds them"""
    got = {}
    orig = eng._optimizer_step

    def step(active, entered, reduce_events=None):
        for name, shape, refs in model.table:
            g = model.P[name].grad.detach().cpu().clone()
            if len(refs) == 1 or refs[1] == "cls.decoder.weight":
                got[refs[0]] = g
            else:
                rows = shape[0] // len(refs)
                for i, r in enumerate(refs):
                    got[r] = g[i * rows:(i + 1) * rows]
        return orig(active, entered, reduce_events)
    eng._optimizer_step = step
    return got


# (below the gather: 1/M of the full-batch gradient, applied to the gathered features: the full gradient)
QUIRKS = {
    "clip": (("clip_model.text_projection", "clip_model.transformer.resblocks.0.attn.in_proj_weight", "clip_model.token_embedding.weight"),
             ("text_fine_weight.0.weight", "clip_model.logit_scale")),
    "swin": (("contra_head_t.linear.weight", "contra_head_v.linear.weight"), ("text_fine_weight.0.weight", "contra_temp")),
    "coarse": (("clip_model.text_projection", "clip_model.transformer.resblocks.0.attn.in_proj_weight", "clip_model.token_embedding.weight"),
               ("va_fusion.weight", "clip_model.logit_scale")),
}


def _check_reference_semantics(dev, variant, M, task):
    spec, sd, full = _setup(variant, M)
    want_losses, want_grads, full_contra, full_grads = _expect(variant, M, task)
    model, eng = _engine(spec, sd, dev)
    try:
        batches = [_part(full, m) for m in range(M)]
        _seed_masker_per_micro_batch(model, batches, 100)
        got = _grads_before_the_step(model, eng)
        out = eng.train_window(batches, task)
        torch.cuda.synchronize()
        res = {k: float(v) for k, v in out.items()}
        flat = model.arena.flat.detach().cpu()
    finally:
        _teardown(model, eng)
    print(f"[window {variant} M={M} {task}] got {res} oracle contra {full_contra} ranks {want_losses}")
    assert eng.global_step == 1 and not eng._window_open and torch.isfinite(flat).all()
    assert set(res) == set(want_losses[0]) | {"total_loss"}
    assert abs(res["contra_loss"] - full_contra) <= 1e-4 * abs(full_contra), (res["contra_loss"], full_contra)
    for r in range(M):           # identical on every rank by construction: each rank's oracle value is the full-batch one too
        assert abs(want_losses[r]["contra_loss"] - full_contra) <= 1e-4 * abs(full_contra)
    total = res["contra_loss"]
    for k in want_losses[0]:
        if k == "contra_loss":
            continue
        want = sum(w[k] for w in want_losses) / M
        assert abs(res[k] - want) <= 1e-4 * abs(want), (k, res[k], want)
        total += res[k]
    assert abs(res["total_loss"] - total) <= 1e-5 * abs(total)
    bad = []
    for k in want_grads[0]:
        parts = [g[k] for g in want_grads if g[k] is not None]
        g = got[k].double()
        if not parts:
            assert float(g.abs().max()) == 0.0, k
            continue
        want = sum(p.double() for p in parts) / M
        scale = max(float(want.norm()), 1e-5 * want.numel() ** 0.5)
        err = float((g.reshape(want.shape) - want).norm()) / scale
        if err > 2e-3:
            bad.append((k, err))
    assert not bad, bad[:8]
    below, above = QUIRKS[variant]
    for k in below:
        g, want = got[k].double(), full_grads[k].double() / M
        assert float(want.norm()) > 0 and float((g.reshape(want.shape) - want).norm()) <= 2e-3 * float(want.norm()), k
    for k in above:
        g, want = got[k].double(), full_grads[k].double()
        assert float(want.norm()) > 0 and float((g.reshape(want.shape) - want).norm()) <= 2e-3 * float(want.norm()) + 1e-9, k
    return res


@pytest.mark.parametrize("M", [2, 4])
def test_window_matches_the_reference_at_world_M(dev, M):
    _check_reference_semantics(dev, "clip", M, TASK)


def test_retrieval_task_window(dev):
    """'ret%tva%tv': no contra_loss_ratio, no decoder -- the training passes have no loss of their own, only the injected slices"""
    res = _check_reference_semantics(dev, "clip", 2, "ret%tva%tv")
    assert set(res) == {"contra_loss", "total_loss"} and res["contra_loss"] == res["total_loss"]


def test_coarse_contrastive_window(dev):
    """contra_type='coarse': pooled features (2-D bank rows), va_fusion applied to the gathered features"""
    _check_reference_semantics(dev, "coarse", 2, TASK)


def test_videoswin_window(dev):
    """VideoSwin + shared-BERT text encoder (the text pass and the decoder write the same arena slots)"""
    _check_reference_semantics(dev, "swin", 2, TASK)


def test_one_micro_batch_is_train_step_to_the_bit(dev):
    spec, sd, full = _setup("clip", 1)
    snaps = []
    for window in (False, True):
        model, eng = _engine(spec, sd, dev)
        try:
            random.seed(5)
            out = eng.train_window([full], TASK) if window else eng.train_step(full, TASK)
            torch.cuda.synchronize()
            snaps.append(({k: v.detach().clone() for k, v in out.items()}, model.arena.flat.detach().clone(), random.getstate(), eng.global_step))
        finally:
            _teardown(model, eng)
    (la, fa, ra, sa), (lb, fb, rb, sb) = snaps
    assert list(la) == list(lb)
    for k in la:
        assert torch.equal(la[k], lb[k]), (k, float(la[k]), float(lb[k]))
    assert torch.equal(fa, fb), int((fa != fb).sum())
    assert ra == rb and sa == sb == 1


class _Recorder(dict):
    """a `collect` hook that keeps every features update"""

    def __init__(self):
        super().__init__()
        self.feats = []

    def update(self, *a, **kw):
        if "feat_t" in kw:
            self.feats.append({k: kw[k].detach().clone() for k in ("feat_t", "feat_v", "feat_a") if kw[k] is not None})
        super().update(*a, **kw)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager_host_rng", "graphs_device_rng"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_training_pass_replays_the_feature_pass(dev, dtype, graphs):
    """dropout 0.1: the features micro-batch m's training pass produces are the bank rows its feature pass produced, to the bit -- over
    three windows (graphs on: the encoders run eagerly in the first, are captured in the second and replayed from then on; the feature
    pass always runs eagerly), then once more through the `collect` hook. The host masker ends where M plain steps leave it."""
    from valor_amd import ops
    M = 2
    spec, sd, full = _setup("clip", M)
    batches = [_part(full, m) for m in range(M)]
    for b in batches:
        b["video_pixels"], b["audio_spectrograms"] = b["video_pixels"].to(dev), b["audio_spectrograms"].to(dev)
    model, eng = _engine(spec, sd, dev, dtype=dtype, dropout=0.1, graphs=graphs)
    try:
        assert (ops.DropoutState.base is not None) == graphs
        ops.DropoutState.reset(11)
        random.seed(21)
        eng.keep_window = True
        for step in range(3):
            out = eng.train_window(batches, TASK)
            bank, feats = eng.last_window["bank"], eng.last_window["train_feats"]
            assert len(feats) == M
            for m in range(M):
                for k in ("feat_t", "feat_v", "feat_a"):
                    assert torch.equal(feats[m][k], bank[k].detach()[m * B_LOCAL:(m + 1) * B_LOCAL]), (step, m, k)
            assert all(bool(torch.isfinite(v)) for v in out.values())
        if graphs:
            assert sorted(model._graph_segs) == ["ast", "clip_text", "decoder", "vit"] and all(s.captured for s in model._graph_segs.values())
        # the rows of different micro-batches come from different dropout windows: the same clip twice gives different features
        twice = eng.feature_pass([batches[0], batches[0]], TASK)[0]
        assert not torch.equal(twice[0].feat_a, twice[1].feat_a)          # (the AST encoder has dropout; the CLIP towers have none)
        rng_after_windows = random.getstate()
        model.collect = rec = _Recorder()
        eng.train_window(batches, TASK)
        model.collect = None
        assert len(rec.feats) == 2 * M                    # M feature passes, then M training passes
        bank = eng.last_window["bank"]
        for m in range(M):
            for k in ("feat_t", "feat_v", "feat_a"):
                assert torch.equal(rec.feats[M + m][k], rec.feats[m][k]), (m, k)
                assert torch.equal(rec.feats[M + m][k], bank[k].detach()[m * B_LOCAL:(m + 1) * B_LOCAL]), (m, k)
        # the masker: the three windows of M micro-batches consumed what 3 * M plain steps consume
        random.seed(21)
        for step in range(3):
            for m in range(M):
                eng.train_step(batches[m], TASK)
        assert random.getstate() == rng_after_windows
    finally:
        model.collect = None
        _teardown(model, eng)


def test_stochastic_depth_factors_are_replayed(dev):
    """VideoSwin with drop_path 0.2 and dropout 0.1: the training pass draws the feature pass's stochastic-depth factors (numpy's global
    generator) again, and the generator ends where M plain steps leave it"""
    from valor_amd import ops
    M = 2
    spec, sd, full = _setup("swin", M)
    batches = [_part(full, m) for m in range(M)]
    model, eng = _engine(spec, sd, dev, dropout=0.1, drop_path=0.2)
    try:
        ops.DropoutState.reset(11)
        random.seed(21)
        np.random.seed(31)
        eng.keep_window = True
        eng.train_window(batches, TASK)
        bank, feats = eng.last_window["bank"], eng.last_window["train_feats"]
        for m in range(M):
            for k in ("feat_t", "feat_v", "feat_a"):
                assert torch.equal(feats[m][k], bank[k].detach()[m * B_LOCAL:(m + 1) * B_LOCAL]), (m, k)
        after = np.random.get_state()
        np.random.seed(31)
        for m in range(M):
            eng.train_step(batches[m], TASK)
        plain = np.random.get_state()
        assert after[2] == plain[2] and np.array_equal(after[1], plain[1])
    finally:
        _teardown(model, eng)


def test_one_contrastive_evaluation_per_window(dev, monkeypatch):
    """3 contrastive groups, M = 4: the fine contrastive kernels run 3 times per window (plain accumulation runs them 12 times), on all
    N rows"""
    from valor_amd import ops
    M = 4
    spec, sd, full = _setup("clip", M)
    calls = []
    orig = ops.fine_contrastive

    def counting(featA, *a, **kw):
        calls.append(featA.shape[0])
        return orig(featA, *a, **kw)
    monkeypatch.setattr(ops, "fine_contrastive", counting)
    model, eng = _engine(spec, sd, dev)
    try:
        batches = [_part(full, m) for m in range(M)]
        random.seed(1)
        eng.train_window(batches, TASK)
        assert calls == [M * B_LOCAL] * 3
        del calls[:]
        for m in range(M):
            eng.train_step(batches[m], TASK, accum_steps=M)
        assert calls == [B_LOCAL] * (3 * M)
    finally:
        _teardown(model, eng)


def test_window_is_not_plain_accumulation(dev):
    """M = 2 on the same seeded data: the window's contra_loss is the oracle's full-batch value, not the mean of the two micro-batches' own
    contrastive losses (which plain accumulation optimises). Two more negatives per row add positive terms to every InfoNCE denominator
    (about ln 2 on unrelated features), so the two must be further apart than ten times the parity tolerance of 1e-4. Guards against a
    silent fallback to accumulation."""
    M = 2
    spec, sd, full = _setup("clip", M)
    _, _, full_contra, _ = _expect("clip", M, TASK)
    model, eng = _engine(spec, sd, dev)
    try:
        batches = [_part(full, m) for m in range(M)]
        with torch.no_grad():                             # each micro-batch's own contrastive loss, at the same parameters
            own = [float(model(batches[m], task="pt_contra%tva%tv%ta", compute_loss=True)["contra_loss"]) for m in range(M)]
        random.seed(100)
        win = float(eng.train_window(batches, TASK)["contra_loss"])
    finally:
        _teardown(model, eng)
    mean_own = sum(own) / M
    print(f"[window vs accumulation] window {win} own {own} oracle full batch {full_contra}")
    assert abs(win - full_contra) <= 1e-4 * abs(full_contra)
    assert abs(win - mean_own) > 1e-3 * abs(mean_own), (win, mean_own)             # ten times the parity tolerance
