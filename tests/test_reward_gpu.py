"""The device caption reward on the GPU (valor_caption_reward, csrc/reward.hip, through scst.DeviceCaptionScorer): per-row CIDEr-D,
BLEU-4 and their sum against the unmodified reference's recorded values (tests/golden/scst_reward.pt) and against the host CaptionScorer
at the bench geometry (256 rows over 64 clips of 20 references, L = 30 and L = 128, rows without eos, rows with eos first, rows with
out-of-range ids); clips of 40 references, whose lists the kernel probes in global memory, mixed with small ones in one launch; NaN for
rows without a clip; determinism and strided input; the rewards of a whole SCST step with the host and with the device scorer; and the
device-reward plumbing of scst_loss.

Tolerance of the fp64 comparisons: rtol 1e-9, atol 1e-12 (the reasoning is in tests/test_reward_cpu.py's docstring: reordered sums of
< 1e3 non-negative terms move by ~1e-13 relative, exp / sqrt / pow by a few ulp). No row is excluded from any comparison."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
EOS = 102


def _goldens():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_reward_goldens
    return make_reward_goldens


def _report(tag, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    rel = err / np.maximum(np.abs(want), 1e-300)
    print(f"[reward {tag}] rows {got.size}: max |d| = {err.max():.3g}, max rel (|want| > 1e-6) = "
          f"{(rel[np.abs(want) > 1e-6].max() if (np.abs(want) > 1e-6).any() else 0.0):.3g}, range {want.min():.4g} .. {want.max():.4g}")


def test_reward_matches_the_reference_fixture(dev):
    from valor_amd import scst
    fix = _goldens().load()
    dsc = scst.DeviceCaptionScorer(fix["refs"], df_ids=fix["df_ids"], device=dev)
    rw, c, b = (t.cpu().numpy() for t in dsc.score(fix["ids"], fix["seq"].to(dev), fix["eos"], parts=True))
    want_c, want_b = fix["cider"].numpy(), fix["bleu4"].numpy()
    _report("fixture CIDEr-D", c, want_c)
    _report("fixture BLEU-4", b, want_b)
    np.testing.assert_allclose(c, want_c, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(b, want_b, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(rw, want_c + want_b, rtol=RTOL, atol=ATOL)
    only = dsc.score(fix["ids"], fix["seq"].to(dev), fix["eos"]).cpu().numpy()          # without the optional outputs: the same reward
    assert np.array_equal(only, rw)


def _bench_case(L, seed=0, clips=64, R=256, vocab=3000):
    """the tools/gen_bench.py 'scst' geometry: 20 references of 6-14 tokens per clip; R rows of width L: random hypotheses, references
    with noise, rows without eos, rows with eos at position 0, rows with ids outside the vocabulary"""
    rng = np.random.default_rng(seed)
    ids_all = [f"clip{i}" for i in range(clips)]
    refs = {i: [rng.integers(1000, vocab, size=int(rng.integers(6, 15))).tolist() for _ in range(20)] for i in ids_all}
    ids = [ids_all[r % clips] for r in range(R)]
    seq = rng.integers(1000, vocab, size=(R, L)).astype(np.int64)
    for r in range(R):
        kind = r % 8
        cr = refs[ids[r]]
        if kind in (1, 2, 5):                                                  # a reference (or two in a row for the wide matrix), then eos
            h = list(cr[int(rng.integers(20))])
            if kind == 2:
                h = h[:int(rng.integers(2, len(h)))] + rng.integers(1000, vocab, size=3).tolist()
            if kind == 5 and L >= 64:
                h = (h + list(cr[int(rng.integers(20))]) + h)[:L - 1]
            h = h[:L - 1]
            seq[r, :len(h)] = h
            seq[r, len(h)] = EOS
        elif kind == 3:
            seq[r, 0] = EOS                                                    # eos first: the empty hypothesis
        elif kind == 4:
            seq[r, int(rng.integers(1, L))] = EOS                              # random tokens, eos somewhere
        elif kind == 6:                                                        # ids outside the vocabulary inside a reference: unmatched
            h = list(cr[0])[:L - 1]
            seq[r, :len(h)] = h
            seq[r, 1] = vocab + 7 if r % 16 == 6 else -3
            seq[r, 2] = 70000
            seq[r, 3] = 70000 if r % 16 == 6 else 80000
            if len(h) < L:
                seq[r, len(h)] = EOS
        # kinds 0 and 7: no eos at all, the whole row counts (kind 7: a reference repeated to the full width)
        if kind == 7:
            h = list(cr[1])
            seq[r] = (h * (L // len(h) + 1))[:L]
    return refs, ids, seq


@pytest.mark.parametrize("L", [30, 128])
def test_reward_matches_the_host_scorer_at_the_bench_geometry(dev, L):
    from valor_amd import scst
    vocab = 3000
    refs, ids, seq = _bench_case(L, seed=L, vocab=vocab)
    assert (seq != EOS).all(axis=1).sum() >= 32 and (seq[:, 0] == EOS).sum() >= 16 and ((seq >= vocab) | (seq < 0)).any(axis=1).sum() >= 16
    host = scst.CaptionScorer(refs)
    dsc = host.to_device(dev, vocab=vocab)
    hyps = scst.hypotheses(seq, EOS)
    want_c = np.array([host.cider(i, h) for i, h in zip(ids, hyps)])
    want_b = np.array([host.bleu4(i, h) for i, h in zip(ids, hyps)])
    rw, c, b = (t.cpu().numpy() for t in dsc.score(ids, torch.from_numpy(seq).to(dev), EOS, parts=True))
    _report(f"L={L} CIDEr-D", c, want_c)
    _report(f"L={L} BLEU-4", b, want_b)
    np.testing.assert_allclose(c, want_c, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(b, want_b, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(rw, host(ids, hyps), rtol=RTOL, atol=ATOL)
    assert np.ptp(want_c) > 0.25 and (want_c[3::8] == 0).all()          # one of 20 references matched whole: CIDEr-D ~0.5
    # the numpy walker of the same tables agrees as well (table format == kernel)
    np.testing.assert_allclose(rw, scst.reward_from_tables(dsc.tables, dsc.clip_index(ids), seq, EOS, vocab=vocab), rtol=RTOL, atol=ATOL)


def test_reward_of_clips_too_large_for_the_lds_stage(dev):
    """clips of 40 references of 12-15 tokens (MSVD has about 40 per clip) carry more than the 1536 reference entries the kernel stages in
    LDS and are probed in global memory; every third clip is one, the others are the bench geometry's 20 references of 6-14 tokens, and
    both kinds are scored in ONE launch. Per-row CIDEr-D, BLEU-4 and the sum against the host CaptionScorer."""
    from valor_amd import scst
    vocab, clips, R, L, STAGE = 3000, 48, 192, 30, 1536
    rng = np.random.default_rng(11)
    names = [f"clip{i}" for i in range(clips)]
    refs = {n: [rng.integers(1000, vocab, size=int(rng.integers(12, 16) if i % 3 == 0 else rng.integers(6, 15))).tolist()
                for _ in range(40 if i % 3 == 0 else 20)] for i, n in enumerate(names)}
    ids = [names[(r * 7) % clips] for r in range(R)]                           # big and small clips interleaved row by row
    seq = rng.integers(1000, vocab, size=(R, L)).astype(np.int64)
    for r in range(R):
        cr, kind = refs[ids[r]], (r // 3) % 4                                  # r // 3: every kind meets big and small clips
        if kind == 0:                                                          # a reference itself
            h = list(cr[int(rng.integers(len(cr)))])
        elif kind == 1:                                                        # a prefix plus noise
            h = list(cr[int(rng.integers(len(cr)))])
            h = h[:int(rng.integers(2, len(h)))] + rng.integers(1000, vocab, size=3).tolist()
        elif kind == 2:                                                        # two references in a row, the first repeated
            h = list(cr[0]) + list(cr[len(cr) - 1])
        else:                                                                  # random tokens, no eos (r % 8 == 1: the empty hypothesis)
            h = [] if r % 8 == 1 else None
        if h is not None:
            h = h[:L - 1]
            seq[r, :len(h)] = h
            seq[r, len(h)] = EOS
    host = scst.CaptionScorer(refs)
    dsc = host.to_device(dev, vocab=vocab)
    T = dsc.tables
    entries = np.array([T["ref_key_ptr"][T["clip_ref_ptr"][c + 1]] - T["ref_key_ptr"][T["clip_ref_ptr"][c]] for c in range(clips)])
    idx = dsc.clip_index(ids)
    big = np.arange(clips) % 3 == 0
    print(f"[reward large clips] entries per clip: large {entries[big].min()} .. {entries[big].max()}, small {entries[~big].min()} .. {entries[~big].max()}")
    assert (entries[big] > STAGE).all() and (entries[~big] <= STAGE).all()     # both branches of the kernel, by construction
    assert big[idx].sum() >= 48 and (~big[idx]).sum() >= 96
    hyps = scst.hypotheses(seq, EOS)
    want_c = np.array([host.cider(i, h) for i, h in zip(ids, hyps)])
    want_b = np.array([host.bleu4(i, h) for i, h in zip(ids, hyps)])
    rw, c, b = (t.cpu().numpy() for t in dsc.score(ids, torch.from_numpy(seq).to(dev), EOS, parts=True))
    for tag, rows in (("large", big[idx]), ("small", ~big[idx])):
        _report(f"{tag} clips CIDEr-D", c[rows], want_c[rows])
        _report(f"{tag} clips BLEU-4", b[rows], want_b[rows])
    np.testing.assert_allclose(c, want_c, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(b, want_b, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(rw, host(ids, hyps), rtol=RTOL, atol=ATOL)
    assert want_c[big[idx]].max() > 0.2 and want_b[big[idx]].max() > 0.9      # the large clips' rows score: a matched reference among 40
    again = dsc.score(ids, torch.from_numpy(seq).to(dev), EOS).cpu().numpy()
    assert np.array_equal(again, rw)                                           # the same bits from the global-memory probes too


def test_rows_without_a_clip_score_nan_and_bad_geometry_raises(dev):
    """valor_caption_reward's contract for table indices handed in directly (score() takes int32 indices unchecked): an index outside
    [0, n_clips) or a clip without references gives NaN in all three outputs and leaves the other rows alone. Geometry the kernel does not
    take raises ValueError in Python, with the limit named."""
    from valor_amd import scst
    refs, ids, seq = _bench_case(30, seed=3, clips=8, R=16)
    refs = dict(refs, bare=[])
    dsc = scst.DeviceCaptionScorer(refs, device=dev, vocab=3000)
    s = torch.from_numpy(seq).to(dev)
    good = dsc.clip_index(ids)
    n_clips = len(dsc.tables["clips"])
    assert dsc.clip_of["bare"] == n_clips - 1
    idx = good.copy()
    idx[[1, 6, 11, 12]] = [-1, n_clips, n_clips - 1, np.iinfo(np.int32).max]
    nan_rows = np.zeros(16, dtype=bool)
    nan_rows[[1, 6, 11, 12]] = True
    want = [t.cpu().numpy() for t in dsc.score(good, s, EOS, parts=True)]
    got = [t.cpu().numpy() for t in dsc.score(idx, s, EOS, parts=True)]
    for g, w in zip(got, want):
        assert np.isnan(g[nan_rows]).all() and np.array_equal(g[~nan_rows], w[~nan_rows]) and not np.isnan(w).any()
    np.testing.assert_allclose(got[0], scst.reward_from_tables(dsc.tables, idx, seq, EOS, vocab=3000), rtol=RTOL, atol=ATOL, equal_nan=True)
    wide = torch.full((16, scst.MAX_ROW_LEN + 1), 1234, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match=str(scst.MAX_ROW_LEN)):
        dsc.score(good, wide, EOS)
    with pytest.raises(ValueError, match="eos"):
        dsc.score(good, s, 3000)
    with pytest.raises(ValueError, match="vocabulary"):
        dsc.score(good, s, EOS, vocab=scst.MAX_VOCAB + 1)
    with pytest.raises(ValueError, match="vocabulary"):
        dsc.advantages(ids, [s], [s], EOS, vocab=70000)
    assert dsc.score(good, wide[:, :scst.MAX_ROW_LEN], EOS).shape == (16,)    # the widest row is inside the domain


def test_reward_is_deterministic_and_takes_strided_rows(dev):
    from valor_amd import scst
    refs, ids, seq = _bench_case(30, seed=7)
    dsc = scst.DeviceCaptionScorer(refs, device=dev, vocab=3000)
    s = torch.from_numpy(seq).to(dev)
    a = [t.clone() for t in dsc.score(ids, s, EOS, parts=True)]
    b = dsc.score(ids, s, EOS, parts=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                               # bit-identical
    wide = torch.full((seq.shape[0], 47), 1234, dtype=torch.int64, device=dev)
    view = wide[:, 9:39]
    view.copy_(s)
    assert not view.is_contiguous() and view.stride(0) == 47
    for x, y in zip(a, dsc.score(ids, view, EOS, parts=True)):
        assert torch.equal(x, y)
    every_other = torch.stack((s, s + 1), dim=1).reshape(-1, 30)[::2]          # row pitch 60
    assert not every_other.is_contiguous() and torch.equal(every_other, s)
    assert torch.equal(dsc.score(ids, every_other, EOS), a[0])
    assert not torch.isnan(a[0]).any()
    with pytest.raises(KeyError):
        dsc.score(["nowhere"] * seq.shape[0], s, EOS)


def _model(spec, dev, sd, **opts):
    from valor_amd.model.valor import VALOR
    m = VALOR({"dropout": 0.0, "drop_path_rate": 0.0, "max_generation_len": 10, "scst_finetuning": True, "seed": 7, **opts}, spec=spec,
              dtype=torch.float32, device=dev)
    m.load_state_dict(sd, strict=True)
    m.train()
    return m


def _batch(spec, b=4, seed=6):
    from valor_amd import synth
    batch = synth.make_batch(spec, batch=b, frames=2, audio_slices=2, txt_len=16, seed=seed)
    batch["ids"] = [f"clip{i}" for i in range(b)]
    return batch


def _scst_step(spec, dev, sd, batch, scorer):
    from valor_amd import decode
    m = _model(spec, dev, sd)
    m.scorer = scorer
    m.collect = {}
    out = m(batch, task="cap%tva%tv", compute_loss=True)
    sum(out.values()).backward()
    torch.cuda.synchronize()
    col = m.collect
    m.collect = None
    decode.release_sessions(m)
    return {k: float(v.detach()) for k, v in out.items()}, col


def test_scst_step_rewards_host_and_device_scorer(dev):
    """a cap%tva%tv SCST step (tiny model, fp32) with the host scorer and with the device scorer under the same sampler seed: identical
    samples and greedy rows, every collected fp32 reward within 1 fp32 ulp of the host path's. The references are cut from what the
    model itself decodes (plus noise), so that the rewards are not all ~0."""
    from valor_amd import scst, synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    batch = _batch(spec)
    b = len(batch["ids"])
    rng = np.random.default_rng(0)
    probe = scst.CaptionScorer({i: [rng.integers(1000, 1040, size=6).tolist()] for i in batch["ids"]})
    _, col = _scst_step(spec, dev, sd, batch, probe)
    refs = {}
    for r, cid in enumerate(batch["ids"]):
        s = scst.hypotheses(col["scst_samples"]["tva"][0].cpu(), EOS)[r]
        g = scst.hypotheses(col["scst_greedy"]["tv"], EOS)[r]
        refs[cid] = [s[:6] + rng.integers(1000, 1100, size=3).tolist(), g[2:] + [1001], (s[3:] + g[:4]) or [1002], rng.integers(1000, 1100, size=8).tolist()]
    host = scst.CaptionScorer(refs)
    loss_h, col_h = _scst_step(spec, dev, sd, batch, host)
    loss_d, col_d = _scst_step(spec, dev, sd, batch, host.to_device(dev))
    for g in ("tva", "tv"):
        assert torch.equal(col_h["scst_samples"][g][0], col_d["scst_samples"][g][0]) and torch.equal(col_h["scst_samples"][g][1], col_d["scst_samples"][g][1])
        assert torch.equal(col_h["scst_greedy"][g], col_d["scst_greedy"][g])
        rd = col_d["scst_rewards"][g]
        assert torch.is_tensor(rd) and rd.is_cuda and rd.dtype == torch.float32 and rd.shape == (b,)
        want = np.asarray(col_h["scst_rewards"][g], dtype=np.float32)
        got = rd.cpu().numpy()
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(got)))
        print(f"[scst step {g}] host fp32 rewards {want}, device {got}, |d| / ulp {np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp}")
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (g, want, got)
    assert any(float(np.abs(np.asarray(col_h["scst_rewards"][g])).max()) > 0.1 for g in ("tva", "tv"))          # rewards that mean something
    for k in loss_h:
        print(f"[scst step] {k}: host scorer {loss_h[k]:.8g}, device scorer {loss_d[k]:.8g}")
        assert np.isfinite(loss_h[k]) and np.isfinite(loss_d[k])


def test_scst_loss_takes_device_rewards_bit_identically(dev):
    """scst_loss with a device fp32 reward tensor and with the same tensor copied to numpy: same weights, same kernels, the same bits"""
    from valor_amd import decode, synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    batch = _batch(spec, b=3)
    groups = ["tva", "tv"]
    gen = torch.Generator().manual_seed(3)
    rw = {g: (torch.randn(3, generator=gen) * 1.7).to(dev) for g in groups}
    res = []
    for form in ("device", "numpy", "mixed"):
        m = _model(spec, dev, sd)
        m.zero_grad()
        vo, ao = m.scst_encode(batch, groups)
        samples = m.scst_sample(vo, ao, groups, seed=5)
        if form == "device":
            r = dict(rw)
        elif form == "numpy":
            r = {g: t.cpu().numpy() for g, t in rw.items()}
        else:
            r = {"tva": rw["tva"], "tv": rw["tv"].cpu().numpy()}
        out = m.scst_loss(vo, ao, {g: samples[g][0] for g in groups}, r)
        sum(out.values()).backward()
        torch.cuda.synchronize()
        res.append(({k: v.detach().clone() for k, v in out.items()}, m.arena.grad.clone()))
        decode.release_sessions(m)
    for other in res[1:]:
        for k in res[0][0]:
            assert torch.equal(res[0][0][k], other[0][k]), k
        assert torch.equal(res[0][1], other[1])
    assert all(float(v) != 0.0 for v in res[0][0].values()) and float(res[0][1].abs().max()) > 0
