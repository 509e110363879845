"""GPU: video patch dropout (valor_amd/csrc/patchdrop.hip and its way through ops, the model, the engine, exact resume and the window
step). The subset draw is held to the host law bit for bit (tests/patch_keep_ref.py); the two data-movement kernels to the gathered rows
of the full kernels bit for bit; the encoder to the same function composed from the existing ops."""
import gc
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import patch_keep_ref as PR

pytestmark = pytest.mark.gpu
TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
VIS = "clip_model.visual."


@pytest.fixture(autouse=True)
def rng_modes(dev):
    from valor_amd import ops
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    yield
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    gc.collect()


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


# ---------------------------------------------------------------------------------------------- 1. the subset draw
def _keep(dev, N, Pn, k, group, seed, offset, base=None):
    from valor_amd import lib
    idx = torch.full((N, k), -7, dtype=torch.int32, device=dev)
    slot = torch.full((N, Pn), -7, dtype=torch.int32, device=dev)
    lib.call("valor_patch_keep", torch.cuda.current_stream().cuda_stream, N, Pn, k, group, seed, offset,
             0 if base is None else base.data_ptr(), idx.data_ptr(), slot.data_ptr())
    return idx.cpu().numpy(), slot.cpu().numpy()


@pytest.mark.parametrize("shape", [(3, 16, 1, 1), (3, 16, 15, 1), (2, 16, 16, 1), (5, 196, 98, 1), (4, 196, 98, 2), (2, 576, 144, 1)],
                         ids=lambda s: "N%d_Pn%d_k%d_g%d" % s)
def test_patch_keep_is_the_host_law(dev, shape):
    N, Pn, k, group = shape
    seed = 0x1234_5678_9ABC
    # by value only
    off = 1000
    idx, slot = _keep(dev, N, Pn, k, group, seed, off)
    want = PR.patch_keep_host(seed, off, N, Pn, k, group)
    assert np.array_equal(idx, want[0]) and np.array_equal(slot, want[1])
    again = _keep(dev, N, Pn, k, group, seed, off)
    assert np.array_equal(idx, again[0]) and np.array_equal(slot, again[1])
    # a device counter of 2^40 + 7; the by-value offset puts the counters' low words across 2^32 inside the first group
    B = (1 << 40) + 7
    base = torch.tensor([B], dtype=torch.int64, device=dev)
    off = (1 << 32) - 7 - Pn // 2
    assert (off + B) % (1 << 32) < (1 << 32) - 1 and ((off + B) % (1 << 32)) + Pn > (1 << 32)
    idx, slot = _keep(dev, N, Pn, k, group, seed, off, base)
    want = PR.patch_keep_host(seed, off + B, N, Pn, k, group)
    assert np.array_equal(idx, want[0]) and np.array_equal(slot, want[1])
    again = _keep(dev, N, Pn, k, group, seed, off, base)
    assert np.array_equal(idx, again[0]) and np.array_equal(slot, again[1])


def test_ops_patch_keep_draws_through_dropout_state(dev):
    from valor_amd import ops
    ops.DropoutState.reset(99, 500)
    idx, slot = ops.patch_keep(4, 16, 8, group=2, device=dev)
    assert ops.DropoutState.offset == 500 + 2 * 16                   # (N / group) * Pn counters
    want = PR.patch_keep_host(99, 500, 4, 16, 8, 2)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(slot.cpu().numpy(), want[1])
    idx2, _ = ops.patch_keep(4, 16, 8, group=2, device=dev)
    assert np.array_equal(idx2.cpu().numpy(), PR.patch_keep_host(99, 532, 4, 16, 8, 2)[0]) and not torch.equal(idx, idx2)


# ---------------------------------------------------------------------------------------------- 2. patchify(keep=)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("geom", [(16, 64, 0), (14, 56, 592)], ids=["p16_64px", "p14_56px_pad592"])
def test_patchify_kept_equals_the_gathered_rows(dev, dtype, geom):
    from valor_amd import ops
    P, res, pad = geom
    N, Pn, k = 3, (res // P) ** 2, 7
    img = torch.randn((N, 3, res, res), generator=torch.Generator().manual_seed(1)).to(dev)
    ops.DropoutState.reset(5)
    idx, _ = ops.patch_keep(N, Pn, k, device=dev)
    full = ops.patchify(img, P, dtype, pad_to=pad)
    got = ops.patchify(img, P, dtype, pad_to=pad, keep=idx)
    rows = (torch.arange(N, device=dev)[:, None] * Pn + idx.long()).reshape(-1)
    assert got.shape == (N * k, max(pad, 3 * P * P)) and got.dtype == dtype
    assert torch.equal(got, full.index_select(0, rows))
    if pad:
        assert bool((got[:, 3 * P * P:] == 0).all()) and bool((got[:, :3 * P * P] != 0).any())


# ---------------------------------------------------------------------------------------------- 3. assemble_tokens_kept
def _assemble_inputs(dev, dtype, N, Pn, E, seed=2):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(s, generator=g).to(dtype).to(dev)
    return mk(N * Pn, E), mk(E), mk(Pn + 1, E), mk(E), mk(N, Pn + 1, E)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_assemble_kept_forward_equals_the_gathered_rows(dev, dtype, bias):
    from valor_amd import ops
    N, Pn, k, E = 5, 16, 6, 72
    patches, cls, pos, bb, _ = _assemble_inputs(dev, dtype, N, Pn, E)
    ops.DropoutState.reset(6)
    idx, slot = ops.patch_keep(N, Pn, k, device=dev)
    full = ops.assemble_tokens(patches, cls, pos, bb if bias else None, N, Pn)
    prow = (torch.arange(N, device=dev)[:, None] * Pn + idx.long()).reshape(-1)
    got = ops.assemble_tokens_kept(patches.index_select(0, prow).contiguous(), cls, pos, bb if bias else None, idx, slot, N, Pn)
    tok = torch.cat([torch.zeros((N, 1), dtype=torch.long, device=dev), 1 + idx.long()], dim=1)
    want = torch.gather(full, 1, tok[:, :, None].expand(N, 1 + k, E))
    assert got.shape == (N, 1 + k, E) and torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_assemble_kept_backward(dev, dtype):
    """dpatches: the rows of dout, bit for bit. dcls / dpos against an fp64 restatement at the tolerance tests/test_embed_ops_gpu.py:95
    holds valor_assemble_tokens_bwd to (relative L2 1e-5 in fp32, 1.2e-2 in bf16). N = 7 frames: one full group of four partial sums and
    a tail. Position 3 is kept by no frame: exactly 0 (and exactly the old value under accumulate)."""
    from valor_amd import lib
    N, Pn, k, E = 7, 16, 5, 72
    g = torch.Generator().manual_seed(3)
    idx = torch.stack([torch.sort(torch.tensor([p for p in torch.randperm(Pn, generator=g).tolist() if p != 3][:k])).values for _ in range(N)])
    slot = torch.full((N, Pn), -1, dtype=torch.int64)
    slot.scatter_(1, idx, torch.arange(k).expand(N, k))
    dout = torch.randn((N, 1 + k, E), generator=g).to(dtype)
    want_pos = torch.zeros((Pn + 1, E), dtype=torch.float64)
    want_pos[0] = dout[:, 0].double().sum(0)
    for f in range(N):
        want_pos[1 + idx[f]] += dout[f, 1:].double()
    d_dout, d_slot = dout.to(dev), slot.to(torch.int32).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    dt = 0 if dtype == torch.bfloat16 else 1

    def run(accumulate, init):
        dpatch = torch.empty((N * k, E), dtype=dtype, device=dev)
        dpos = torch.full((Pn + 1, E), init, dtype=dtype, device=dev)
        dcls = torch.full((E,), init, dtype=dtype, device=dev)
        lib.call("valor_assemble_tokens_kept_bwd", st, dt, d_dout.data_ptr(), d_slot.data_ptr(), dpatch.data_ptr(), dpos.data_ptr(), dcls.data_ptr(),
                 N, Pn, k, E, accumulate)
        return dpatch, dpos, dcls

    tol = 1e-5 if dtype == torch.float32 else 1.2e-2
    dpatch, dpos, dcls = run(0, 123.0)                        # accumulate = 0 overwrites whatever the buffers held
    assert torch.equal(dpatch, d_dout[:, 1:].reshape(N * k, E))
    print("assemble_kept_bwd rel err", dtype, _rel(dpos.cpu(), want_pos), _rel(dcls.cpu(), want_pos[0]))
    assert _rel(dpos.cpu(), want_pos) < tol and _rel(dcls.cpu(), want_pos[0]) < tol
    assert bool((dpos[1 + 3] == 0).all())
    again = run(0, -5.0)
    assert all(torch.equal(a, b) for a, b in zip((dpatch, dpos, dcls), again))
    _, apos, acls = run(1, 2.0)
    assert _rel(apos.cpu(), want_pos + 2.0) < tol and _rel(acls.cpu(), want_pos[0] + 2.0) < tol
    assert bool((apos[1 + 3] == 2.0).all())


def test_assemble_kept_autograd_without_sinks(dev):
    """the autograd Function on plain leaf tensors (no gradient arena): dcls / dpos / dbias come back through autograd"""
    from valor_amd import ops
    N, Pn, k, E = 4, 16, 8, 64
    patches, cls, pos, bb, _ = _assemble_inputs(dev, torch.float32, N, Pn, E)
    ops.DropoutState.reset(8)
    idx, slot = ops.patch_keep(N, Pn, k, device=dev)
    kept = patches[:N * k].clone().requires_grad_(True)
    cls, pos, bb = (t.requires_grad_(True) for t in (cls, pos, bb))
    out = ops.assemble_tokens_kept(kept, cls, pos, bb, idx, slot, N, Pn)
    dout = torch.randn((N, 1 + k, E), generator=torch.Generator().manual_seed(4)).to(dev)
    out.backward(dout)
    r_kept, r_cls, r_pos, r_bb = (t.detach().double().requires_grad_(True) for t in (kept, cls, pos, bb))
    tok = torch.cat([torch.zeros((N, 1), dtype=torch.long, device=dev), 1 + idx.long()], dim=1)
    ref = torch.cat([r_cls.expand(N, 1, E), r_kept.view(N, k, E) + r_bb], dim=1) + r_pos[tok]
    ref.backward(dout.double())
    assert _rel(out, ref.detach()) < 1e-6
    for a, b in ((kept, r_kept), (cls, r_cls), (pos, r_pos), (bb, r_bb)):
        assert _rel(a.grad, b.grad) < 1e-5               # tests/test_embed_ops_gpu.py:95


# ---------------------------------------------------------------------------------------------- 4. the encoder
def _model(spec, sd, dtype, dev, **opts):
    from valor_amd.model.valor import VALOR
    m = VALOR(dict({"dropout": 0.0}, **opts), spec=spec, dtype=dtype, device=dev)
    m.load_state_dict(sd, strict=True)
    return m.train()


def _vis_grads(model):
    return {n: p.grad.detach().clone() for n, p in model.P.items() if n.startswith(VIS) and p.grad is not None}


def _encoder_pair(dev, spec, dtype, frames, clips, mode, seed=21):
    """-> (kept-path output, composed output, kept-path gradients, composed gradients, k): the composition is full patchify, the conv GEMM,
    assemble_tokens, an index_select of rows [0] + 1 + idx of every frame, LayerNorm and _clip_blocks -- existing ops only"""
    from valor_amd import ops, synth
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    Pn = spec.vis_tokens - 1
    k = Pn // 2
    model = _model(spec, sd, dtype, dev, video_patch_keep=k, video_patch_dropout_mode=mode)
    bn = clips * frames
    imgs = torch.randn((bn, 3, spec.resolution, spec.resolution), generator=torch.Generator().manual_seed(seed)).to(dev)
    ops.DropoutState.reset(31)
    model._pd_group = frames if mode == "tube" else 1
    out = model._video_encoder_clip(imgs)
    idx, slot = model.last_patch_keep
    assert out.shape == (bn, 1 + k, spec.vis_width) and idx.shape == (bn, k) and slot.shape == (bn, Pn)
    want = PR.patch_keep_host(31, 0, bn, Pn, k, model._pd_group)
    assert np.array_equal(idx.cpu().numpy(), want[0])
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed + 1)).to(dtype).to(dev)
    model.arena.grad.zero_()
    out.backward(dout)
    g_kept = _vis_grads(model)
    # the same function from the existing ops
    P = model.P
    model.arena.grad.zero_()
    wconv = ops.param_view(P[VIS + "conv1.weight"], spec.vis_width, -1)
    vec = 8 if dtype == torch.bfloat16 else 4
    kp = (wconv.shape[1] + vec - 1) // vec * vec
    patches = ops.patchify(imgs, spec.patch, dtype, pad_to=kp)
    if kp != wconv.shape[1]:
        wconv = ops.pad_cols(wconv, kp)
    tok = ops.linear(patches, wconv, None)
    x = ops.assemble_tokens(tok, P[VIS + "class_embedding"], P[VIS + "positional_embedding"], None, bn, Pn)
    rows = torch.cat([torch.zeros((bn, 1), dtype=torch.long, device=dev), 1 + idx.long()], dim=1) + torch.arange(bn, device=dev)[:, None] * (Pn + 1)
    x = torch.index_select(x.reshape(bn * (Pn + 1), -1), 0, rows.reshape(-1)).view(bn, 1 + k, -1)
    x = ops.layer_norm(x, P[VIS + "ln_pre.weight"], P[VIS + "ln_pre.bias"], 1e-5)
    ref = model._clip_blocks(x, VIS + "transformer", spec.vis_layers, spec.vis_heads, None, P[VIS + "ln_post.weight"], P[VIS + "ln_post.bias"])
    ref.backward(dout)
    g_ref = _vis_grads(model)
    return out.detach(), ref.detach(), g_kept, g_ref, k


NAMES = ("conv1.weight", "class_embedding", "positional_embedding", "ln_pre.weight", "ln_pre.bias")


@pytest.mark.parametrize("mode", ["frame", "tube"])
@pytest.mark.parametrize("variant", ["tiny", "tiny_clip_bert"])
def test_encoder_equals_its_composition_fp32(dev, variant, mode):
    """fp32: outputs at atol 2e-4 / rtol 1e-4 (tests/test_model_gpu.py:106), every gradient of the visual tower at a relative L2 error of
    2e-3 (tests/test_model_gpu.py:92-94), the bars that file sets between two fp32 evaluations of the model"""
    from valor_amd import synth
    spec = synth.tiny_spec() if variant == "tiny" else synth.tiny_clip_bert_spec()
    out, ref, g_kept, g_ref, k = _encoder_pair(dev, spec, torch.float32, frames=2, clips=2, mode=mode)
    print("encoder fp32 max abs diff", float((out - ref).abs().max()))
    assert torch.allclose(out, ref, atol=2e-4, rtol=1e-4)
    assert set(g_kept) == set(g_ref) and all(VIS + n in g_ref for n in NAMES)
    assert any("resblocks.0." in n for n in g_ref) and any(f"resblocks.{spec.vis_layers - 1}." in n for n in g_ref)
    for n, want in g_ref.items():
        scale = max(float(want.norm()), 1e-5 * want.numel() ** 0.5)
        err = float((g_kept[n] - want).norm()) / scale
        assert err <= 2e-3, (n, err)
        assert float(want.abs().max()) > 0 or n == VIS + "proj", n         # (the projection head is not part of the encoder function)


def test_encoder_equals_its_composition_bf16(dev):
    """bf16 at the base widths (b = 2, F = 2, Pn = 196, k = 98): outputs within the ~0.9 % relative L2 error tests/test_model_gpu.py:325
    states for bf16 encoder outputs, per-tensor gradients within the 3 % of tests/test_model_gpu.py:415 (held here on the norm of the
    difference, which bounds that file's difference of norms)"""
    from valor_amd import synth
    spec = synth.shallow_base_spec()
    out, ref, g_kept, g_ref, k = _encoder_pair(dev, spec, torch.bfloat16, frames=2, clips=2, mode="frame")
    assert k == 98
    print("encoder bf16 rel", _rel(out, ref))
    assert _rel(out, ref) <= 9e-3
    assert set(g_kept) == set(g_ref)
    for n, want in g_ref.items():
        assert _rel(g_kept[n], want) <= 0.03, (n, _rel(g_kept[n], want))


# ---------------------------------------------------------------------------------------------- 5. the model
def _tiny(dev, batch=4, frames=2):
    from valor_amd import synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    b = synth.make_batch(spec, batch=batch, frames=frames, audio_slices=2, txt_len=32, seed=4)
    return spec, sd, b


def _train_pass(model, batch, seed=11):
    from valor_amd import ops
    ops.DropoutState.reset(41)
    random.seed(seed)
    model.arena.grad.zero_()
    model.collect = col = {}
    try:
        out = model(batch, task=TASK, compute_loss=True)
    finally:
        model.collect = None
    sum(out.values()).backward()
    torch.cuda.synchronize()
    return out, col, model.arena.grad.detach().clone(), ops.DropoutState.offset


def test_model_trains_on_the_kept_tokens(dev):
    spec, sd, batch = _tiny(dev)
    plain = _model(spec, sd, torch.float32, dev)
    drop = _model(spec, sd, torch.float32, dev, video_patch_dropout=0.5)
    _, _, g_plain, _ = _train_pass(plain, batch)
    out, col, g_drop, _ = _train_pass(drop, batch)
    Pn = spec.vis_tokens - 1
    k = Pn - int(Pn * 0.5)
    assert col["video_output"].shape == (4, 2, 1 + k, spec.vis_width)
    assert set(out) == {"contra_loss", "caption_loss", "mlm_loss"} and all(bool(torch.isfinite(v)) for v in out.values())
    idx, slot = drop.last_patch_keep
    assert idx.shape == (8, k) and slot.shape == (8, Pn)
    for name, (o, cnt, _) in plain.arena.offsets.items():
        if float(g_plain[o:o + cnt].abs().max()) > 0:
            assert float(g_drop[o:o + cnt].abs().max()) > 0, name
    assert bool(torch.isfinite(g_drop).all())


def test_eval_keeps_every_token(dev):
    spec, sd, batch = _tiny(dev)
    outs = []
    for opts in ({}, {"video_patch_dropout": 0.5}):
        m = _model(spec, sd, torch.float32, dev, **opts).eval()
        with torch.no_grad():
            random.seed(12)
            m.collect = col = {}
            ev = m(batch, task=TASK, compute_loss=False)
            m.collect = None
        assert col["video_output"].shape[2] == spec.vis_tokens and m.last_patch_keep is None
        outs.append(ev)
    assert outs[0].keys() == outs[1].keys()
    for key, v in outs[0].items():
        if torch.is_tensor(v):
            assert torch.equal(v, outs[1][key]), key


def test_option_off_is_the_plain_model_to_the_bit(dev):
    from valor_amd import synth
    spec, sd, batch = _tiny(dev)
    runs = []
    for opts in ({}, {"video_patch_dropout": 0.0}, {"video_patch_keep": spec.vis_tokens - 1}, {"video_patch_dropout": 0.0, "video_patch_dropout_mode": "tube"}):
        m = _model(spec, sd, torch.bfloat16, dev, **dict(opts, dropout=0.1))
        out, col, g, off = _train_pass(m, batch)
        assert m.last_patch_keep is None and col["video_output"].shape[2] == spec.vis_tokens
        runs.append(({k: v.detach().clone() for k, v in out.items()}, g, off))
    for out, g, off in runs[1:]:
        assert off == runs[0][2] and torch.equal(g, runs[0][1])
        for k, v in runs[0][0].items():
            assert torch.equal(out[k], v), k


# ---------------------------------------------------------------------------------------------- 6. the engine
def _opts():
    return SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-4, clip_lr_text=1e-4, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0)


def _engine(dev, graphs, weight_seed=3, mode="frame", device_rng=True, dtype=torch.bfloat16, dropout=0.1):
    from valor_amd import ops, synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=weight_seed, w_std=0.05)
    model = VALOR({"dropout": dropout, "video_patch_dropout": 0.5, "video_patch_dropout_mode": mode, "seed": 7}, spec=spec, dtype=dtype, device=dev)
    model.load_state_dict(sd, strict=True)
    eng = TrainEngine(model, _opts(), manage_gc=False, graphs=graphs)
    if dtype != torch.float32:
        eng.optimizer.init_master_from(sd)
    if not graphs and device_rng:
        ops.DropoutState.enable_device_base(dev)            # the eager twin draws from the same device-mode windows
    return spec, model, eng


def _batch(spec, dev, seed, batch=4):
    from valor_amd import synth
    b = synth.make_batch(spec, batch=batch, frames=2, audio_slices=1, txt_len=32, seed=seed)
    b["video_pixels"], b["audio_spectrograms"] = b["video_pixels"].to(dev), b["audio_spectrograms"].to(dev)
    return b


def _teardown(model, eng):
    from valor_amd import ops
    torch.cuda.synchronize()
    model.enable_graphs(False)
    eng.close()
    ops.DropoutState.disable_device_base()


@pytest.mark.parametrize("mode", ["frame", "tube"])
def test_graphed_steps_equal_eager_steps(dev, mode):
    """five training steps with the encoders captured on the third call and replayed, against five eager steps from the same state: the
    parameters and every loss equal to the bit (the property tests/test_graphs_gpu.py holds for the plain model), the tables of every step
    equal, and successive steps draw different tables"""
    from valor_amd import ops
    runs = {}
    for graphs in (False, True):
        spec, model, eng = _engine(dev, graphs, mode=mode)
        batch = _batch(spec, dev, 4)
        ops.DropoutState.reset(77)
        random.seed(5)
        losses, tables = [], []
        for step in range(5):
            out = eng.train_step(batch, TASK)
            losses.append({k: float(v) for k, v in out.items()})
            tables.append(model.last_patch_keep[0].clone())
        torch.cuda.synchronize()
        if graphs:
            assert "vit" in model._graph_segs and len(model._graph_segs["vit"].captured) == 1
            assert next(iter(model._graph_segs["vit"].captured.values())).draws == (4 if mode == "tube" else 8) * 16
        runs[graphs] = (losses, model.arena.flat.clone(), tables)
        _teardown(model, eng)
        del model, eng
    assert runs[False][0] == runs[True][0], (runs[False][0], runs[True][0])
    assert torch.equal(runs[False][1], runs[True][1])
    for a, b in zip(runs[False][2], runs[True][2]):
        assert torch.equal(a, b)
    tabs = runs[True][2]
    assert all(not torch.equal(tabs[i], tabs[i + 1]) for i in range(4))
    if mode == "tube":
        assert all(torch.equal(t[0::2], t[1::2]) for t in tabs)          # the two frames of a clip share a subset


def test_resumed_run_continues_bit_identically(dev, tmp_path):
    """four steps against two steps + save_run + a fresh model, engine and scrambled process state + resume_run + two steps, as
    tests/test_resume_gpu.py holds for the plain model"""
    from valor_amd import checkpoint, ops

    def seed_run(s):
        ops.DropoutState.reset(s)
        random.seed(s + 1)
        np.random.seed(s + 2)
        torch.manual_seed(s + 3)

    def steps(spec, model, eng, first, n):
        snaps = []
        for s in range(first, first + n):
            out = eng.train_step(_batch(spec, dev, 10 + s, batch=2), TASK)
            snaps.append(({k: v.detach().clone() for k, v in out.items()}, model.arena.flat.detach().clone(), eng.optimizer.master.clone(),
                          model.last_patch_keep[0].clone()))
        return snaps

    seed_run(77)
    spec, model, eng = _engine(dev, True)
    want = steps(spec, model, eng, 0, 4)
    _teardown(model, eng)
    del model, eng
    seed_run(77)
    spec, model, eng = _engine(dev, True)
    steps(spec, model, eng, 0, 2)
    checkpoint.save_run(eng, str(tmp_path), blocking=True)
    _teardown(model, eng)
    del model, eng
    seed_run(4000)
    spec, model, eng = _engine(dev, True, weight_seed=11)
    assert checkpoint.resume_run(eng, str(tmp_path)) == 2
    got = steps(spec, model, eng, 2, 2)
    _teardown(model, eng)
    for i in range(2):
        w, g = want[2 + i], got[i]
        assert torch.equal(g[3], w[3]), ("tables", i)
        for k in w[0]:
            assert torch.equal(g[0][k], w[0][k]), (i, k)
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2]), i
    assert not torch.equal(want[2][3], want[3][3])


# ---------------------------------------------------------------------------------------------- 7. the window step
@pytest.mark.parametrize("graphs", [False, True], ids=["eager_host_rng", "graphs_device_rng"])
def test_window_training_pass_draws_the_feature_pass_tables(dev, graphs):
    """train_window with M = 2: the tables of micro-batch m's feature pass and of its training pass are equal, the two micro-batches'
    tables differ; and the training pass's features are the bank rows (what tests/test_window_gpu.py holds for the plain model). Three
    windows: with graphs on the ViT runs eagerly, is captured and is replayed."""
    from valor_amd import ops
    M, B = 2, 2
    spec, model, eng = _engine(dev, graphs, device_rng=False, dtype=torch.float32)
    batches = [_batch(spec, dev, 20 + m, batch=B) for m in range(M)]
    seen = []
    inner = model.forward_video_encoder

    def recording(video_pixels):
        out = inner(video_pixels)
        seen.append((model.last_patch_keep[0].clone(), tuple(out.shape)))
        return out

    model.forward_video_encoder = recording
    try:
        ops.DropoutState.reset(11)
        random.seed(21)
        eng.keep_window = True
        for step in range(3):
            del seen[:]
            out = eng.train_window(batches, TASK)
            assert all(bool(torch.isfinite(v)) for v in out.values())
            assert len(seen) == 2 * M                     # M feature passes, then M training passes
            assert all(shape == (B, 2, 1 + 8, spec.vis_width) for _, shape in seen)
            for m in range(M):
                assert torch.equal(seen[m][0], seen[M + m][0]), (step, m)
            assert not torch.equal(seen[0][0], seen[1][0])
            bank, feats = eng.last_window["bank"], eng.last_window["train_feats"]
            for m in range(M):
                assert torch.equal(feats[m]["feat_v"], bank["feat_v"].detach()[m * B:(m + 1) * B]), (step, m)
        if graphs:
            assert model._graph_segs["vit"].captured
    finally:
        model.forward_video_encoder = inner
        _teardown(model, eng)
