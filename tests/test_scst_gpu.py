"""Self-critical caption finetuning on the GPU: the categorical sampler (valor_sample_tokens) -- its law against softmax, its logP against
fp64, determinism, -inf / NaN / finished rows --; the sampled decode (graph replay == eager step, [SEP] after the first [SEP], a kept
session sees in-place weight updates); the on-policy check (the loss pass's per-token logP equals the sampler's); the reward-weighted
loss (zero reward: zero loss and gradient; a constant reward scales the loss; constant and per-row rewards against the CPU oracle's
full-masker pass with reward_loss restated on its logits, losses and gradients); TrainEngine steps bit-identical with graphs on / off and
with checkpointing on / off."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

EOS = 102
CHI2_DF15_P1E3 = 37.697          # chi-square quantile, 15 degrees of freedom, upper tail 1e-3


def _draw(logits, seed, offset, unfinished=None, eos=EOS):
    from valor_amd import kernels as K
    R = logits.shape[0]
    unf = torch.ones(R, dtype=torch.bool, device=logits.device) if unfinished is None else unfinished
    tok = torch.empty(R, dtype=torch.int64, device=logits.device)
    sents = torch.full((R, 3), -7, dtype=torch.int64, device=logits.device)
    lp = torch.full((R, 3), -7.0, dtype=torch.float32, device=logits.device)
    K.sample_tokens(logits, seed, offset, eos, unf, tok, sents[:, 1], lp[:, 1])
    torch.cuda.synchronize()
    assert torch.equal(tok, sents[:, 1]) and (sents[:, 0] == -7).all() and (sents[:, 2] == -7).all()
    return tok, lp[:, 1], unf


def test_sampler_law_and_logp_v16(dev):
    torch.manual_seed(0)
    row = torch.randn(16, dtype=torch.float64) * 1.5
    R = 16384
    logits = row.float()[None].repeat(R, 1).to(dev)
    tok, lp, unf = _draw(logits, 1234, 0, eos=5)
    t = tok.cpu()
    assert ((t >= 0) & (t < 16)).all()
    p = torch.softmax(row.float().double(), 0).numpy()
    obs = np.bincount(t.numpy(), minlength=16)
    chi2 = float(((obs - R * p) ** 2 / (R * p)).sum())
    assert chi2 < CHI2_DF15_P1E3, (chi2, obs, R * p)
    ref = torch.log_softmax(row.float().double(), 0)[t].numpy()
    assert np.abs(lp.cpu().double().numpy() - ref).max() < 1e-5
    assert torch.equal(unf.cpu(), t != 5)                                       # rows that drew the end token finished, the others not
    tok2, lp2, _ = _draw(logits, 1234, 0, eos=5)
    assert torch.equal(tok, tok2) and torch.equal(lp, lp2)                     # a pure function of (seed, offset, row, column)
    tok3, _, _ = _draw(logits, 1234, R * 4, eos=5)
    assert not torch.equal(tok, tok3)


def test_sampler_law_vocab_dominant(dev):
    V, R = 30522, 8192
    g = torch.Generator().manual_seed(3)
    row = torch.randn(V, generator=g, dtype=torch.float64) * 0.5
    top = [17, 4000, 30000]
    row[top] = torch.tensor([9.0, 8.5, 8.0], dtype=torch.float64)
    logits = torch.zeros((R, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :V]
    logits.copy_(row.float()[None].expand(R, V))
    tok, lp, _ = _draw(logits, 99, 5)
    t = tok.cpu().numpy()
    p = torch.softmax(row.float().double(), 0).numpy()
    cats = top + [-1]
    pc = np.array([p[c] for c in top] + [1 - p[top].sum()])
    oc = np.array([(t == c).sum() for c in top] + [np.isin(t, top, invert=True).sum()])
    chi2 = float(((oc - R * pc) ** 2 / (R * pc)).sum())
    assert chi2 < 16.27, (chi2, oc, R * pc, cats)                              # 3 degrees of freedom, upper tail 1e-3
    ref = torch.log_softmax(row.float().double(), 0)[torch.from_numpy(t)].numpy()
    assert np.abs(lp.cpu().double().numpy() - ref).max() < 1e-5


def test_sampler_never_draws_a_column_far_behind(dev):
    """u is never 1 (the odd multiples of 2^-24 in (0, 1)): a column 40 logits behind the leader has probability e^-40 per draw, so over
    8192 rows of V = 30522 no other column may ever be drawn (a uniform that rounds to 1 would give a column key +inf whatever its logit)"""
    V, R = 30522, 8192
    g = torch.Generator().manual_seed(4)
    row = torch.randn(V, generator=g) * 0.1
    row[12345] = 40.0
    logits = torch.zeros((R, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :V]
    logits.copy_(row[None].expand(R, V))
    for off in (0, 1 << 33):
        tok, lp, _ = _draw(logits, 2024 + off, off)
        assert (tok == 12345).all(), int((tok != 12345).sum())
        assert float(lp.abs().max()) < 1e-5


def test_sampler_edge_rows(dev):
    V = 300
    logits = torch.randn((6, V), device=dev)
    logits[0, :] = -float("inf")
    logits[0, 7] = 0.0                                                   # only column 7 is drawable
    logits[1, ::2] = -float("inf")                                       # -inf columns never drawn
    logits[2, 11] = float("nan")                                         # NaN row: EOS, NaN logP, finished
    logits[3, EOS] = 80.0                                                # draws EOS: finishes
    unfinished = torch.tensor([1, 1, 1, 1, 0, 1], dtype=torch.bool, device=dev)       # row 4 finished before
    tok, lp, unf = _draw(logits, 7, 0, unfinished)
    tok, lp, unf = tok.cpu(), lp.cpu(), unf.cpu()
    assert tok[0] == 7 and abs(float(lp[0])) < 1e-6
    assert tok[1] % 2 == 1
    assert tok[2] == EOS and torch.isnan(lp[2]) and not unf[2]
    assert tok[3] == EOS and not unf[3]
    assert tok[4] == EOS and lp[4] == 0.0 and not unf[4]
    assert ((tok >= 0) & (tok < V)).all() and unf[0] and unf[1] and unf[5]
    for _ in range(200):                                                 # many draws of row 1: never an -inf column
        t, _, _ = _draw(logits[1:2].contiguous(), int(torch.randint(0, 2 ** 62, ())), 0)
        assert int(t) % 2 == 1


def _model(spec, dtype, dev, **opts):
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05, bf16_exact=dtype == torch.bfloat16)
    m = VALOR({"dropout": 0.0, "drop_path_rate": 0.0, "max_generation_len": 10, **opts}, spec=spec, dtype=dtype, device=dev)
    m.load_state_dict(sd, strict=True)
    return m


def _release(m):
    """drop the model's decoding sessions now: a session and its model reference each other, and a cycle that holds captured graphs must
    not be left to the garbage collector, which may run in the middle of a later test's graph capture"""
    from valor_amd import decode
    decode.release_sessions(m)


def _batch(spec, b=3, seed=6, bf16=False):
    from valor_amd import synth
    batch = synth.make_batch(spec, batch=b, frames=2, audio_slices=2, txt_len=16, seed=seed, bf16_exact=bf16)
    batch["ids"] = [f"clip{i}" for i in range(b)]
    return batch


def test_sampled_decode_graph_equals_eager_and_sees_weight_updates(dev, monkeypatch):
    from valor_amd import decode, synth
    spec = synth.tiny_spec()
    m = _model(spec, torch.float32, dev)
    batch = _batch(spec)
    outs = []
    for graph in ("1", "0"):
        monkeypatch.setenv("VALOR_DECODE_GRAPH", graph)
        decode.release_sessions(m)
        outs.append({k: v.cpu() for k, v in decode.generate_cap(m, batch, ["tva", "tv"], mode="sample", seed=11).items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    for key in ("t_va", "t_v"):
        s, lp = outs[0]["generated_sequences_" + key], outs[0]["logprobs_" + key]
        for r in range(s.shape[0]):
            hit = (s[r] == EOS).nonzero()
            if hit.numel():
                j = int(hit[0])
                assert (s[r, j:] == EOS).all() and (lp[r, j + 1:] == 0).all()
        assert torch.isfinite(lp).all() and (lp <= 0).all()
    # a kept (graph-captured) session after an in-place update of the arena (what the fused AdamW does) == a fresh session
    monkeypatch.setenv("VALOR_DECODE_GRAPH", "1")
    decode.release_sessions(m)
    decode.generate_cap(m, batch, ["tva"], mode="sample", seed=3)
    decode.generate_cap(m, batch, ["tva"], mode="sample", seed=3)         # captured by now
    with torch.no_grad():
        m.arena.flat.add_(torch.randn_like(m.arena.flat) * 0.01)
    kept = decode.generate_cap(m, batch, ["tva"], mode="sample", seed=3)
    monkeypatch.setenv("VALOR_DECODE_GRAPH", "0")
    decode.release_sessions(m)
    fresh = decode.generate_cap(m, batch, ["tva"], mode="sample", seed=3)
    _release(m)
    for k in kept:
        assert torch.equal(kept[k].cpu(), fresh[k].cpu()), k


def _on_policy(m, batch, groups):
    m.train()
    m.collect = {}
    vo, ao = m.scst_encode(batch, groups)
    samples = m.scst_sample(vo, ao, groups, seed=21)
    b = vo.shape[0]
    losses = m.scst_loss(vo, ao, {g: samples[g][0] for g in groups}, {g: np.ones(b) for g in groups})
    rows = m.collect["scst_loss_rows"][0]
    m.collect = None
    _release(m)
    diffs, r0 = [], 0
    for g in groups:
        s, lp = samples[g]
        _, lab = m.scst_inputs(s.cpu())
        keep = lab != -1
        n = int(keep.sum())
        want = lp.cpu()[keep[:, -s.shape[1] - 1:-1] if m.caption_type == "unimlm" else keep[:, :s.shape[1]]]
        got = -rows[r0:r0 + n].cpu()
        diffs.append(float((got - want).abs().max()))
        assert abs(float(losses["caption_loss_" + g]) - float(rows[r0:r0 + n].mean())) < 1e-4 * max(1.0, float(rows[r0:r0 + n].mean()))
        r0 += n
    return max(diffs)


@pytest.mark.parametrize("prompt", [False, True])
@pytest.mark.parametrize("caption_type", ["unimlm", "lm"])
def test_on_policy_logp_fp32(dev, caption_type, prompt):
    """the sampler's per-token logP == the log-probability the SCST loss pass assigns to the same token (rewards 1): the two-stream
    layout reproduces the decoding conditionals"""
    from valor_amd import synth
    spec = synth.tiny_spec()
    m = _model(spec, torch.float32, dev, caption_type=caption_type, use_task_prompt=prompt)
    d = _on_policy(m, _batch(spec), ["tva", "tv", "ta"])
    print(f"[on-policy fp32 {caption_type} prompt={prompt}] max |dlogP| = {d:.3g}")
    assert d < 1e-4


BF16_LOGP_BAND = 0.1


def test_on_policy_logp_bf16(dev):
    from valor_amd import synth
    spec = synth.shallow_base_spec("clip")
    m = _model(spec, torch.bfloat16, dev)
    d = _on_policy(m, _batch(spec, b=4, bf16=True), ["tva", "tv"])
    print(f"[on-policy bf16] max |dlogP| = {d:.3g} (band {BF16_LOGP_BAND})")
    assert d < BF16_LOGP_BAND


def test_reward_scaling_and_zero_reward(dev):
    """reward c: the loss is c x the reward-1 loss and the gradients c x; reward 0: loss exactly 0, zero gradient"""
    from valor_amd import synth
    spec = synth.tiny_spec()
    m = _model(spec, torch.float32, dev)
    batch = _batch(spec)
    groups = ["tva", "tv"]
    res = {}
    for c in (1.0, 2.5, 0.0):
        m.train()
        m.zero_grad()
        vo, ao = m.scst_encode(batch, groups)
        samples = m.scst_sample(vo, ao, groups, seed=5)
        out = m.scst_loss(vo, ao, {g: samples[g][0] for g in groups}, {g: np.full(vo.shape[0], c) for g in groups})
        sum(out.values()).backward()
        torch.cuda.synchronize()
        res[c] = ({k: float(v) for k, v in out.items()}, m.arena.grad.clone())
    _release(m)
    for k in res[1.0][0]:
        assert abs(res[2.5][0][k] - 2.5 * res[1.0][0][k]) <= 1e-5 * abs(res[2.5][0][k])
        assert res[0.0][0][k] == 0.0
    g1, g25 = res[1.0][1].float(), res[2.5][1].float()
    assert float((g25 - 2.5 * g1).norm()) <= 2e-3 * float(g25.norm()) and float(g1.norm()) > 0
    assert float(res[0.0][1].abs().max()) == 0.0


def _engine_run(spec, sd, dev, graphs, ckpt, steps=4):
    from types import SimpleNamespace
    from valor_amd import decode, ops, scst
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    m = VALOR({"dropout": 0.1, "drop_path_rate": 0.0, "max_generation_len": 8, "scst_finetuning": True, "checkpointing": ckpt, "seed": 7},
              spec=spec, dtype=torch.float32, device=dev)
    m.load_state_dict(sd, strict=True)
    rng = np.random.default_rng(0)
    m.scorer = scst.CaptionScorer({f"clip{i}": [rng.integers(1000, 1040, size=6).tolist() for _ in range(3)] for i in range(3)})
    opts = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-4, clip_lr_text=1e-4, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0)
    eng = TrainEngine(m, opts, manage_gc=False, graphs=graphs)
    eng.optimizer.init_master_from(sd)
    if not graphs:
        ops.DropoutState.enable_device_base(dev)            # the eager twin draws from the same device-mode windows
    ops.DropoutState.reset(77)
    enc0 = m.P["clip_model.visual.conv1.weight"].detach().clone()
    losses = []
    for s in range(steps):
        out = eng.train_step(_batch(spec, seed=10 + s), "cap%tva%tv")
        losses.append({k: float(v) for k, v in out.items()})
    torch.cuda.synchronize()
    res = (losses, m.arena.flat.detach().clone(), not torch.equal(enc0, m.P["clip_model.visual.conv1.weight"]))
    if graphs:
        assert "decoder" in m._graph_segs and len(m._graph_segs["decoder"].captured) >= 1
    m.enable_graphs(False)
    decode.release_sessions(m)
    eng.close()
    ops.DropoutState.disable_device_base()
    return res


def test_engine_steps_graphs_and_checkpointing(dev):
    """four TrainEngine steps of cap%tva%tv with scst_finetuning and a real CaptionScorer: losses and parameters bit-identical with graphs
    on and off and with checkpointing on and off; the encoders move; a second run reproduces the first"""
    from valor_amd import ops, synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    try:
        base = _engine_run(spec, sd, dev, graphs=True, ckpt=False)
        assert base[2]                                                       # the encoders receive gradient
        assert all(np.isfinite(v) for l in base[0] for v in l.values()) and {"caption_loss_tva", "caption_loss_tv"} <= set(base[0][0])
        for graphs, ckpt in ((False, False), (False, True), (True, False)):
            l, p, _ = _engine_run(spec, sd, dev, graphs=graphs, ckpt=ckpt)
            assert l == base[0], (graphs, ckpt, l, base[0])
            assert torch.equal(p, base[1]), (graphs, ckpt)
    finally:
        ops.DropoutState.disable_device_base()
        ops.DropoutState.reset(1234)


@pytest.mark.parametrize("rewards", ["constant", "per_row"])
def test_scst_loss_and_gradients_match_the_oracle(dev, rewards):
    """the SCST loss pass against the CPU oracle (fp32, tiny spec, cap%tva%tv, dropout 0; the pattern of
    tests/test_finetune_gpu.py::test_full_masker_finetune_losses_match_oracle): the oracle runs its full-masker caption pass on
    [CLS, sequence up to its first [SEP], padding] -- the labelled rows are the positions reward_loss keeps -- and reward_loss
    (pretrain.py:166-173) is restated on its logits: mean over the labelled rows of -r_row * logP. constant: c times the oracle's caption
    loss; per_row: a different reward per sequence. Losses within 1e-4 relative, every parameter's gradient within 2e-3 relative norm."""
    import torch.nn.functional as F
    from valor_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import valor_oracle as VO
    from test_model_gpu import _native_grads
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    batch = synth.make_batch(spec, batch=3, frames=2, audio_slices=1, txt_len=16, seed=5)
    b, L, groups = 3, 8, ["tva", "tv"]
    gen = torch.Generator().manual_seed(9)
    seqs = {}
    for gi, g in enumerate(groups):
        s = torch.randint(1000, 1200, (b, L), generator=gen)
        for r, e in enumerate(((3, 0, None), (None, 5, 0))[gi]):      # first [SEP] at e (None: the sequence never ends)
            if e is not None:
                s[r, e:] = EOS
        seqs[g] = s
    if rewards == "constant":
        rw = {g: np.full(b, 1.7) for g in groups}
    else:
        rw = {"tva": np.array([0.7, -1.3, 2.1]), "tv": np.array([-0.4, 1.9, 0.25])}
    # native
    model = _model(spec, torch.float32, dev)
    model.load_state_dict(sd, strict=True)
    model.train()
    model.zero_grad()
    vo, ao = model.scst_encode(batch, groups)
    out = model.scst_loss(vo, ao, seqs, rw)
    sum(out.values()).backward()
    torch.cuda.synchronize()
    # oracle
    sd_o = VO.trainable_copy(sd)
    orc = VO.Oracle(spec, sd_o, vocab_tokens=synth.synthetic_vocab(spec.vocab), full_masker=True)
    vout = orc.forward_video_encoder(batch["video_pixels"])
    aout = orc.forward_audio_encoder(batch["audio_spectrograms"])
    vi, ai = orc.multimodal_inputs(vout, aout, b)
    ref = {}
    for g in groups:
        s = seqs[g]
        txt = torch.cat((torch.full((b, 1), 101, dtype=torch.long), s), dim=1)
        for r in range(b):                                           # everything behind the first [SEP] becomes padding
            hit = (s[r] == EOS).nonzero()
            if hit.numel():
                txt[r, int(hit[0]) + 2:] = 0
        tin, tlab = orc.caption_inputs(txt)
        o = orc.bert_model(tin, None, vi, ai if "a" in g else None, True, True)
        sel = tlab != -1
        scores = orc.cls_head(o[:, :tin.shape[1]][sel])
        ce = F.cross_entropy(scores, tlab[sel], reduction="none")
        rows = sel.nonzero(as_tuple=True)[0]
        r_row = torch.as_tensor(rw[g], dtype=torch.float32)[rows]
        ref[g] = (r_row * ce).mean()
        if rewards == "constant":
            assert abs(float(ref[g]) - 1.7 * float(ce.mean())) <= 1e-5 * abs(float(ref[g]))
    sum(ref.values()).backward()
    for g in groups:
        a, n = float(ref[g]), float(out["caption_loss_" + g])
        assert abs(a - n) <= 1e-4 * abs(a), (g, a, n)
    ng = _native_grads(model)
    bad = []
    for k, p in sd_o.items():
        if VO.is_alias_key(k) or not p.is_floating_point() or p.grad is None:
            continue
        go, gn = p.grad, ng[k].detach().cpu()
        scale = max(float(go.norm()), 1e-5 * go.numel() ** 0.5)
        if float((gn.reshape(go.shape) - go).norm()) / scale > 2e-3:
            bad.append((k, float((gn.reshape(go.shape) - go).norm()) / scale))
    assert not bad, bad[:8]
