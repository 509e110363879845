"""The device token masker (valor_amd/csrc/masker.hip, valor_amd/model/valor.py DeviceTokenMasker): the two kernels
bit-exact against a numpy restatement of the algorithm, its invariants, its distribution against the reference masker's law
(modeling.py:134-174), and the model / training engine in token_masker='device' mode computing exactly what the host path computes on
the same masks."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dropout_ref import philox4x32_10

pytestmark = pytest.mark.gpu
TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
MASK, RS = 103, 106
U32 = np.uint64(0xFFFFFFFF)


def ref_mask_tokens(tokens, k, seed, offset, mask_token, rs, re):
    b, T = tokens.shape
    out, lab = tokens.copy(), np.full_like(tokens, -1)
    for i in range(b):
        cand = np.flatnonzero(tokens[i, 1:]) + 1
        w0, w1, w2, w3 = philox4x32_10(seed, np.uint64(offset) + np.uint64(i * T) + cand.astype(np.uint64))
        key = w0 | (w1 << np.uint64(32))
        order = np.lexsort((cand, key))                       # smallest key first, ties by position
        for q in order[:min(max(int(k[i]), 0), cand.size)]:
            j = cand[q]
            lab[i, j] = tokens[i, j]
            if w2[q] < 3435973836:
                out[i, j] = mask_token
            elif w2[q] < 3865470566:
                out[i, j] = rs + int((int(w3[q]) * (re - rs)) >> 32)
    return out, lab


def ref_masked_rows(labels, G, Ttot, r0):
    b = labels.shape[0]
    bi, tj = np.nonzero(labels != -1)
    idx = np.concatenate([r0 + (g * b + bi) * Ttot + tj for g in range(G)])
    return idx, np.tile(labels[bi, tj], G)


def synthetic_tokens(b, T, seed, vocab=30522, ones=2, holes=True):
    """[CLS] w .. w [SEP] 0 .. 0 rows of random lengths; the first `ones` rows have a single candidate; `holes`: a few interior zeros"""
    g = np.random.default_rng(seed)
    t = np.zeros((b, T), dtype=np.int64)
    for i in range(b):
        L = 2 if i < ones else int(g.integers(3, T + 1))
        t[i, 0] = 101
        t[i, 1:L] = g.integers(RS, vocab, size=L - 1)
        if L >= 3:
            t[i, L - 1] = 102
        if holes and i >= ones and L > 6 and g.random() < 0.3:
            t[i, int(g.integers(2, L - 1))] = 0
    return t


def _masker(dev, seed=42, vocab=30522):
    from valor_amd.model.valor import DeviceTokenMasker
    return DeviceTokenMasker(MASK, RS, vocab, lambda t: t.to(dev), seed=seed)


@pytest.mark.parametrize("T", [32, 42, 512])
def test_kernels_bit_exact_against_numpy(dev, T):
    from valor_amd import kernels as K
    b = 37
    toks = synthetic_tokens(b, T, seed=T)
    m = np.count_nonzero(toks[:, 1:], axis=1)
    g = np.random.default_rng(T + 1)
    k = np.array([int(g.integers(1, mi + 1)) for mi in m], dtype=np.int32)
    k[5] = m[5] + 3                                            # clamped to the row's candidates
    seed, offset = 0x9E3779B97F4A7C15, (1 << 40) + 12345
    out, lab = K.mask_tokens(torch.from_numpy(toks).to(dev), torch.from_numpy(k).to(dev), seed, offset, MASK, RS, 30522)
    want_out, want_lab = ref_mask_tokens(toks, k, seed, offset, MASK, RS, 30522)
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(lab.cpu().numpy(), want_lab)
    assert int((lab[5] != -1).sum()) == m[5]
    counts = (want_lab != -1).sum(axis=1)
    n = int(counts.sum())
    off = torch.from_numpy((np.cumsum(counts) - counts).astype(np.int32)).to(dev)
    for G, Ttot, r0 in ((1, T, 0), (3, T + 9, 7777)):
        idx, labs = K.masked_rows(lab, off, n, G, Ttot, r0)
        want_idx, want_labs = ref_masked_rows(want_lab, G, Ttot, r0)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(labs.cpu().numpy(), want_labs)
        # a slice of a larger buffer: nothing outside it is written
        big = torch.full((G * n + 10,), -7, dtype=torch.int64, device=dev)
        K.masked_rows(lab, off, n, G, Ttot, r0, idx=big[5:5 + G * n], lab_out=torch.empty(G * n, dtype=torch.int64, device=dev))
        assert (big[:5] == -7).all() and (big[5 + G * n:] == -7).all() and np.array_equal(big[5:5 + G * n].cpu().numpy(), want_idx)


def test_masked_rows_never_writes_past_its_offsets(dev):
    """offsets that undercount a row: the row stops at the next row's offset (and the last row at n)"""
    from valor_amd import kernels as K
    lab = torch.full((3, 32), -1, dtype=torch.int64, device=dev)
    lab[:, 1:9] = 500                                           # 8 labels per row
    off = torch.tensor([0, 4, 8], dtype=torch.int32, device=dev)   # claims 4 per row
    buf = torch.full((2 * 12 + 4,), -9, dtype=torch.int64, device=dev)
    K.masked_rows(lab, off, 12, 2, 40, 0, idx=buf[:24], lab_out=torch.empty(24, dtype=torch.int64, device=dev))
    got = buf.cpu().numpy()
    assert (got[24:] == -9).all()
    assert list(got[:4]) == [1, 2, 3, 4] and list(got[4:8]) == [41, 42, 43, 44] and list(got[12:16]) == [3 * 40 + 1 + j for j in range(4)]


@pytest.mark.parametrize("p", [0.15, 0.6, 0.99])
def test_invariants(dev, p):
    from valor_amd import kernels as K
    b, T, V = 64, 32, 30522
    toks = synthetic_tokens(b, T, seed=3)
    mk = _masker(dev)
    for _ in range(5):
        out, ml = mk(torch.from_numpy(toks), p)
        o, lab = out.cpu().numpy(), ml.labels.cpu().numpy()
        sel = lab != -1
        assert np.array_equal(sel.sum(axis=1), ml.counts)                      # exactly k_i labels per row
        assert (ml.counts >= 1).all()
        assert not sel[:, 0].any() and not sel[toks == 0].any()                # position 0 and padding never touched
        assert np.array_equal(o[~sel], toks[~sel]) and np.array_equal(lab[sel], toks[sel])
        r = o[sel]
        assert ((r == MASK) | ((r >= RS) & (r < V)) | (r == toks[sel])).all()
        assert np.array_equal(ml.src.numpy(), toks)
        idx, labs = K.masked_rows(ml.labels, ml.offsets, ml.n, 1, T, 0)
        bi, tj = np.nonzero(sel)                                               # the order of nonzero() of the device labels
        assert np.array_equal(idx.cpu().numpy(), bi * T + tj) and np.array_equal(labs.cpu().numpy(), lab[sel])
    assert mk.calls == 5 and mk.offset == 5 * b * T


def test_distribution(dev):
    """2000 calls at a fixed seed: per-position selection frequency p / (1 - (1-p)^m), the 80 / 10 / 10 split and the random-token
    histogram (64 bins) within 6 sigma"""
    b, T, V = 64, 32, 30522
    R = V - RS
    toks = synthetic_tokens(b, T, seed=11)
    m = np.count_nonzero(toks[:, 1:], axis=1)
    tt = torch.from_numpy(toks).to(dev)
    edges = (np.arange(65) * R) // 64                                          # bin q = [edges[q], edges[q+1]) of token - RS
    width = np.diff(edges)
    for p, calls in ((0.15, 2000), (0.6, 1000)):
        mk = _masker(dev, seed=5)
        hits = torch.zeros((b, T), dtype=torch.int64, device=dev)
        n_mask = torch.zeros((), dtype=torch.int64, device=dev)
        n_keep = torch.zeros((), dtype=torch.int64, device=dev)
        hist = torch.zeros(64, dtype=torch.int64, device=dev)
        e_dev = torch.from_numpy(edges[1:-1]).to(dev)
        for _ in range(calls):
            out, ml = mk(torch.from_numpy(toks), p)
            sel = ml.labels != -1
            hits += sel
            n_mask += (sel & (out == MASK)).sum()
            n_keep += (sel & (out == tt)).sum()
            rnd = out[sel & (out != MASK) & (out != tt)] - RS
            hist += torch.bincount(torch.bucketize(rnd, e_dev, right=True), minlength=64)
        hits, n_sel = hits.cpu().numpy(), int(hits.sum())
        q = p / (1 - (1 - p) ** m)
        cand = np.zeros((b, T), dtype=bool)
        cand[:, 1:] = toks[:, 1:] != 0
        exp = np.broadcast_to(q[:, None], (b, T))[cand] * calls
        sd = np.sqrt(exp * (1 - exp / calls))
        assert (np.abs(hits[cand] - exp) <= 6 * sd + 1e-9).all()
        assert (hits[~cand] == 0).all()
        # split: [MASK] 0.8, kept 0.1 (+ a random token that equals the original: 0.1 / R), random the rest
        for cnt, pr in ((int(n_mask), 0.8), (int(n_keep), 0.1 + 0.1 / R)):
            assert abs(cnt - pr * n_sel) <= 6 * np.sqrt(n_sel * pr * (1 - pr)), (p, cnt, pr, n_sel)
        h = hist.cpu().numpy().astype(np.float64)
        e = width / R * h.sum()
        chi2 = float(((h - e) ** 2 / e).sum())
        assert chi2 < 63 + 6 * np.sqrt(2 * 63), (p, chi2)


def test_streams_differ_by_call_and_rank_and_repeat_by_seed(dev, monkeypatch):
    from valor_amd.model import valor as vm
    toks = torch.from_numpy(synthetic_tokens(64, 32, seed=2))
    a, b = _masker(dev, seed=8), _masker(dev, seed=8)
    a0, a1 = a(toks, 0.15), a(toks, 0.15)
    b0, b1 = b(toks, 0.15), b(toks, 0.15)
    for (x_out, x_lab), (y_out, y_lab) in ((a0, b0), (a1, b1)):
        assert torch.equal(x_out, y_out) and torch.equal(x_lab.labels, y_lab.labels) and np.array_equal(x_lab.counts, y_lab.counts)
    assert not torch.equal(a0[1].labels, a1[1].labels)                         # another call index: another mask
    monkeypatch.setattr(vm, "_dp_rank", lambda: 1)
    r0 = _masker(dev, seed=8)(toks, 0.15)
    assert not torch.equal(r0[1].labels, a0[1].labels)                         # another rank: another mask
    assert not torch.equal(_masker(dev, seed=9)(toks, 0.15)[1].labels, r0[1].labels)


# ------------------------------------------------------------------ the model: device mode == the host path on the same masks
def _record(model):
    """wrap the device masker: every draw is kept (host copies of its tokens / labels, in call order)"""
    draws, inner = [], model.device_masker

    def rec(tokens, p):
        out, ml = inner(tokens, p)
        draws.append((out.cpu(), ml.labels.cpu()))
        return out, ml
    model.device_masker = rec
    return draws


def _replay(model, draws):
    """host mode whose TokenMasker returns the recorded draws"""
    it = iter(list(draws))
    model.device_masker = None
    model.text_masker = lambda tokens, p: next(it)


def _grads(model):
    return model.arena.grad.detach().clone()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("graphs", [False, True])
def test_forward_pt_equals_the_host_path_on_the_same_masks(dev, dtype, graphs, monkeypatch):
    """forward_pt of the bench task (base widths, B = 8): losses and every parameter gradient bit-identical; with graphs the encoders and
    the decoder stack are captured on the third call and replayed on the fourth"""
    from valor_amd import ops, synth
    from valor_amd.model.valor import VALOR
    monkeypatch.setenv("VALOR_MASKER", "device")
    spec = synth.base_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.02)
    model = VALOR({"dropout": 0.1}, spec=spec, dtype=dtype, device=dev)
    model.load_state_dict(sd, strict=True)
    model.train()
    batch = synth.make_batch(spec, batch=8, frames=2, audio_slices=1, txt_len=32, seed=4)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    if graphs:
        model.enable_graphs(True)
    try:
        runs = {}
        draws = _record(model)
        for mode in ("device", "host"):
            if mode == "host":
                _replay(model, draws)
            ops.DropoutState.reset(77)
            state = random.getstate()
            res = []
            for _ in range(4 if graphs else 2):
                model.zero_grad()
                out = model(batch, task=TASK, compute_loss=True)
                sum(out.values()).backward()
                res.append(({k: v.detach().float().cpu() for k, v in out.items()}, _grads(model)))
            torch.cuda.synchronize()
            if mode == "device":
                assert random.getstate() == state                                  # the device masker leaves python's RNG alone
                assert len(draws) == 2 * len(res)                                  # caption + mlm per step
            runs[mode] = res
        if graphs:
            assert "decoder" in model._graph_segs and len(model._graph_segs["decoder"].captured) == 1
        for (ld, gd), (lh, gh) in zip(runs["device"], runs["host"]):
            assert set(ld) == set(lh) == {"contra_loss", "caption_loss", "mlm_loss"}
            for k in ld:
                assert torch.equal(ld[k], lh[k]), (k, ld[k], lh[k])
            assert torch.isfinite(gd.float()).all() and float(gd.float().abs().sum()) > 0
            assert torch.equal(gd, gh)
        assert not torch.equal(runs["device"][0][0]["mlm_loss"], runs["device"][1][0]["mlm_loss"])   # fresh masks every step
    finally:
        model.enable_graphs(False)
        ops.DropoutState.reset(1234)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_forward_cap_and_text_mlm_equal_the_host_path(dev, dtype, monkeypatch):
    from valor_amd import ops, synth
    from valor_amd.model.valor import VALOR
    monkeypatch.setenv("VALOR_MASKER", "device")
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    model = VALOR({"dropout": 0.1}, spec=spec, dtype=dtype, device=dev)
    model.load_state_dict(sd, strict=True)
    model.train()
    batch = synth.make_batch(spec, batch=4, frames=2, audio_slices=1, txt_len=32, seed=6)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    for run in (lambda: model(batch, task="cap%tva%tv", compute_loss=True), lambda: model.text_mlm(batch, compute_loss=True)):
        inner = model.device_masker
        draws = _record(model)
        res = {}
        for mode in ("device", "host"):
            if mode == "host":
                _replay(model, draws)
            ops.DropoutState.reset(55)
            model.zero_grad()
            out = run()
            sum(out.values()).backward()
            res[mode] = ({k: v.detach().float().cpu() for k, v in out.items()}, _grads(model))
        assert len(draws) == 1
        assert set(res["device"][0]) == set(res["host"][0]) and all(torch.equal(res["device"][0][k], res["host"][0][k]) for k in res["host"][0])
        assert torch.equal(res["device"][1], res["host"][1]) and float(res["device"][1].float().abs().sum()) > 0
        model.device_masker = inner
    ops.DropoutState.reset(1234)


def test_host_labelled_caption_beside_device_mlm(dev, monkeypatch):
    """caption_type 'lm' (next-token labels, no masker) with a device-masked mlm pass: the row-batched decoder mixes a host-labelled and a
    device-labelled pass in one index / label buffer, bit-identical to the host path"""
    from valor_amd import ops, synth
    from valor_amd.model.valor import VALOR
    monkeypatch.setenv("VALOR_MASKER", "device")
    spec = synth.tiny_spec()
    model = VALOR({"dropout": 0.1, "caption_type": "lm"}, spec=spec, dtype=torch.float32, device=dev)
    model.load_state_dict(synth.make_state_dict(spec, seed=5, w_std=0.05), strict=True)
    model.train()
    batch = synth.make_batch(spec, batch=4, frames=2, audio_slices=1, txt_len=32, seed=6)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    draws = _record(model)
    res = {}
    for mode in ("device", "host"):
        if mode == "host":
            _replay(model, draws)
        ops.DropoutState.reset(55)
        model.zero_grad()
        out = model(batch, task="pt_caption%tva%tv_mlm%tva", compute_loss=True)
        sum(out.values()).backward()
        res[mode] = ({k: v.detach().float().cpu() for k, v in out.items()}, _grads(model))
    ops.DropoutState.reset(1234)
    assert len(draws) == 1 and set(res["device"][0]) == {"caption_loss", "mlm_loss"}
    assert all(torch.equal(res["device"][0][k], res["host"][0][k]) for k in res["host"][0])
    assert torch.equal(res["device"][1], res["host"][1])


def test_evaluation_outputs_device_labels(dev, monkeypatch):
    """compute_loss=False in device mode: txt_labels_* are the device labels and evaluate.validate_pt consumes them"""
    from valor_amd import evaluate, synth
    from valor_amd.model.valor import VALOR
    monkeypatch.setenv("VALOR_MASKER", "device")
    spec = synth.tiny_spec()
    model = VALOR({"dropout": 0.0}, spec=spec, dtype=torch.float32, device=dev)
    model.load_state_dict(synth.make_state_dict(spec, seed=5, w_std=0.05), strict=True)
    batch = synth.make_batch(spec, batch=4, frames=2, audio_slices=1, txt_len=32, seed=6)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    model.eval()
    with torch.no_grad():
        ev = model(batch, task="pt_caption%tva%tv_mlm%tva", compute_loss=False)
    for tag in ("caption", "mlm"):
        lab = ev[f"txt_labels_{tag}"]
        assert lab.is_cuda and lab.shape == batch["txt_tokens"]["bert_tokens"].shape
        assert ev[f"{tag}_scores_tva"].shape[0] == int((lab != -1).sum())
    log = evaluate.validate_pt(model, [batch], "pt_caption%tva%tv_mlm%tva")
    assert {"caption_acc_tva", "caption_acc_tv", "mlm_acc_tva"} <= set(log)


# ------------------------------------------------------------------ the training engine
def _engine_run(dev, graphs, steps=3):
    from valor_amd import ops, synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    model = VALOR({"dropout": 0.1, "token_masker": "device", "seed": 17}, spec=spec, dtype=torch.bfloat16, device=dev)
    model.load_state_dict(sd, strict=True)
    opts = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-4, clip_lr_text=1e-4, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0)
    eng = TrainEngine(model, opts, manage_gc=False, graphs=graphs)
    eng.optimizer.init_master_from(sd)
    if not graphs:
        ops.DropoutState.enable_device_base(dev)            # the eager twin draws from the same device-mode windows
    batch = synth.make_batch(spec, batch=4, frames=2, audio_slices=1, txt_len=32, seed=4)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    ops.DropoutState.reset(77)
    random.seed(5)
    losses = []
    for _ in range(steps):
        state = random.getstate()
        out = eng.train_step(batch, TASK)
        assert random.getstate() == state
        losses.append({k: float(v) for k, v in out.items()})
    torch.cuda.synchronize()
    flat = model.arena.flat.clone()
    model.enable_graphs(False)
    eng.close()
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)
    return losses, flat


def test_engine_steps_in_device_mode(dev, monkeypatch):
    monkeypatch.delenv("VALOR_MASKER", raising=False)
    graphed = _engine_run(dev, True)
    again = _engine_run(dev, True)
    eager = _engine_run(dev, False)
    assert all(np.isfinite(v) for step in graphed[0] for v in step.values())
    assert graphed[0] == again[0] and torch.equal(graphed[1], again[1])          # two fresh runs, one seed
    assert graphed[0] == eager[0] and torch.equal(graphed[1], eager[1])          # graphed == eager (VALOR_GRAPHS=0)
    assert len({l["mlm_loss"] for l in graphed[0]}) == 3
