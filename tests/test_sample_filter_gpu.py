"""Caption sampling filters on the GPU (valor_sample_tokens_filtered): filters off == valor_sample_tokens bit for bit; top-k exact
against a host sort (ties at the threshold, -inf columns, k at and above the column count); top-k 1 == arg max; the nucleus on rows
whose fp64 boundary is known; the draw of every filtered case == valor_sample_tokens on the row masked with the kernel's own cut; the
drawn distribution; determinism; buffer neighbours. Then generate_cap: default == filters given as off == the unfiltered loop,
top_k 1 x 4 sequences == greedy, several sequences per clip, graphs on / off, the re-run path, a kept session under other settings,
the model's sample_* options."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

EOS = 102
INF = float("inf")
CHI2_DF4_P1E3 = 18.467           # chi-square quantile, 4 degrees of freedom, upper tail 1e-3
# The kernel's mass error (the sandwich of the flat nucleus cases). A column's mass is floor(expf(y - max) * 2^40) summed in 64-bit
# integers: truncation < 2^-40 per column, at most 49408 * 2^-40 = 4.5e-8 of the leader's mass (M >= 1); expf is 1 ulp (1.2e-7
# relative); the fp32 rounding of y - max changes a column's mass by at most 6e-8 * |d| e^-|d| <= 2.2e-8 of the leader's. Both the
# running mass and M carry these: the ratio compared with top_p is within 2 * (1.2e-7 + 4.5e-8 + 2.2e-8) = 3.8e-7 < DELTA.
DELTA = 1e-6
INV07 = float(torch.tensor(1 / 0.7, dtype=torch.float32))


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def padded(rows, dev, pad_to=32, extra=0):
    """fp32 host rows [R, V] -> device view [R, V] of a zero-padded buffer (row pitch a multiple of pad_to, plus extra)"""
    R, V = rows.shape
    ld = (V + pad_to - 1) // pad_to * pad_to + extra
    buf = torch.zeros((R, ld), dtype=torch.float32, device=dev)[:, :V]
    buf.copy_(rows)
    return buf


def fdraw(logits, seed, offset, inv=1.0, k=0, p=1.0, unfinished=None, eos=EOS, stats=True):
    from valor_amd import kernels as K
    R = logits.shape[0]
    dev = logits.device
    unf = torch.ones(R, dtype=torch.bool, device=dev) if unfinished is None else unfinished.clone()
    tok = torch.empty(R, dtype=torch.int64, device=dev)
    sents = torch.full((R, 3), -7, dtype=torch.int64, device=dev)
    lp = torch.full((R, 3), -7.0, dtype=torch.float32, device=dev)
    kept = torch.full((R,), -7, dtype=torch.int32, device=dev) if stats else None
    cut = torch.full((R,), -7.0, dtype=torch.float32, device=dev) if stats else None
    K.sample_tokens_filtered(logits, seed, offset, eos, unf, tok, sents[:, 1], lp[:, 1], inv, k, p, kept, cut)
    torch.cuda.synchronize()
    assert torch.equal(tok, sents[:, 1]) and (sents[:, 0] == -7).all() and (sents[:, 2] == -7).all()       # neighbours untouched
    assert (lp[:, 0] == -7.0).all() and (lp[:, 2] == -7.0).all()
    assert ((tok >= 0) & (tok < logits.shape[1])).all()
    return tok, lp[:, 1].clone(), unf, kept, cut


def plain(logits, seed, offset, unfinished=None, eos=EOS):
    from valor_amd import kernels as K
    R = logits.shape[0]
    dev = logits.device
    unf = torch.ones(R, dtype=torch.bool, device=dev) if unfinished is None else unfinished.clone()
    tok = torch.empty(R, dtype=torch.int64, device=dev)
    sents = torch.empty(R, dtype=torch.int64, device=dev)
    lp = torch.empty(R, dtype=torch.float32, device=dev)
    K.sample_tokens(logits, seed, offset, eos, unf, tok, sents, lp)
    torch.cuda.synchronize()
    return tok, lp, unf


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_draw(logits, seed, offset, inv, res, eos=EOS):
    """the filtered draw == valor_sample_tokens on where(y >= cut, y, -inf), y the same single multiply, cut the kernel's own"""
    tok, lp, unf, kept, cut = res
    y = logits * torch.tensor(inv, dtype=torch.float32, device=logits.device)
    assert torch.equal(kept.long(), (y >= cut[:, None]).sum(1)), (kept, (y >= cut[:, None]).sum(1))
    masked = padded(torch.where(y >= cut[:, None], y, torch.full_like(y, -INF)), logits.device)
    tok2, lp2, unf2 = plain(masked, seed, offset, eos=eos)
    assert torch.equal(tok, tok2) and torch.equal(unf, unf2)
    assert float((lp - lp2).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ kernel
def test_filters_off_equal_the_plain_sampler_bit_for_bit(dev):
    g = torch.Generator().manual_seed(0)
    cases = [(padded(torch.randn((5, 30522), generator=g) * 2, dev), None),
             (padded(torch.randn((7, 1001), generator=g), dev, pad_to=1, extra=2), None)]              # ld 1003: unaligned rows
    edge = torch.randn((6, 300), generator=g)
    edge[0, :] = -INF
    edge[0, 7] = 0.0
    edge[1, ::2] = -INF
    edge[2, 11] = float("nan")
    edge[3, EOS] = 80.0
    cases.append((edge.to(dev), torch.tensor([1, 1, 1, 1, 0, 1], dtype=torch.bool, device=dev)))
    for logits, unf0 in cases:
        V = logits.shape[1]
        want = plain(logits, 77, 5, unf0)
        for k in (0, V, V + 3):
            for stats in (False, True):                 # False: dispatched to valor_sample_tokens; True: the filtered kernel itself
                tok, lp, unf, kept, cut = fdraw(logits, 77, 5, 1.0, k, 1.0, unf0, stats=stats)
                assert torch.equal(tok, want[0]) and same_bits(lp, want[1]) and torch.equal(unf, want[2]), (V, k, stats)
    # kept / cut of the edge rows: rows that do not draw (NaN, finished before) write 0 / NaN
    tok, lp, unf, kept, cut = fdraw(cases[2][0], 77, 5, 1.0, 0, 1.0, cases[2][1])
    assert kept.tolist() == [1, 150, 0, 300, 0, 300]
    assert float(cut[0]) == 0.0 and torch.isnan(cut[2]) and torch.isnan(cut[4])
    assert float(cut[5]) == float(cases[2][0][5].min())


def topk_rows(V, g):
    rows = torch.randn((4, V), generator=g) * 2
    rows[1] = torch.round(rows[1] * 2) / 2                   # many ties, also at the threshold
    rows[3] = torch.round(rows[3])
    if V > 3:
        rows[2, ::3] = -INF
        rows[3, 1::2] = -INF
    return rows


@pytest.mark.parametrize("V", [1, 5, 1001, 30522, 49408])
def test_top_k_is_exact(dev, V):
    g = torch.Generator().manual_seed(V)
    rows = topk_rows(V, g)
    logits = padded(rows, dev, pad_to=4 if V != 1001 else 1)
    eos = V - 1
    ties_seen = 0
    for temp in (0.5, 1.0, 2.0):
        inv = f32(1.0 / temp)
        y = rows * torch.tensor(inv, dtype=torch.float32)
        vals = torch.sort(y, dim=1, descending=True).values
        nfin = (y > -INF).sum(1)
        for k in (1, 2, 50, V - 1, V, V + 7):
            res = fdraw(logits, 5 + k, 64 * k, inv, k, 1.0, eos=eos)
            kth = torch.stack([vals[r, k - 1] if 1 <= k < int(nfin[r]) else vals[r, int(nfin[r]) - 1] for r in range(4)])
            want_kept = (y >= kth[:, None]).sum(1)
            assert torch.equal(res[4].cpu(), kth), (V, temp, k, res[4].cpu(), kth)
            assert torch.equal(res[3].cpu().long(), want_kept), (V, temp, k)
            ties_seen += int((want_kept > k).sum()) if 1 <= k < int(nfin.min()) else 0
            check_draw(logits, 5 + k, 64 * k, inv, res, eos=eos)
    assert V < 1001 or ties_seen > 0


def test_top_k_1_is_the_arg_max(dev):
    g = torch.Generator().manual_seed(21)
    rows = torch.randn((64, 30522), generator=g)
    top2 = rows.topk(2, dim=1).values
    assert (top2[:, 0] > top2[:, 1]).all()
    logits = padded(rows, dev)
    for seed in (1, 2, 3, 99):
        for inv in (1.0, INV07):
            tok, lp, unf, kept, cut = fdraw(logits, seed, 1000 * seed, inv, 1, 1.0)
            assert torch.equal(tok.cpu(), rows.argmax(1))
            assert (lp == 0).all() and (kept == 1).all()


def test_top_p_exact_cases(dev):
    from test_sample_filter_cpu import DOMINANT_CASES, dominant_row
    row = dominant_row()
    logits = padded(row[None].repeat(3, 1), dev)
    for inv, p, want in DOMINANT_CASES:
        res = fdraw(logits, 31, 7, inv, 0, p)
        assert res[3].tolist() == [want] * 3, (inv, p, res[3].tolist())
        y = row * torch.tensor(inv, dtype=torch.float32)
        assert float(res[4][0]) == float(torch.sort(y, descending=True).values[want - 1])
        check_draw(logits, 31, 7, inv, res)


@pytest.mark.parametrize("V,top_k", [(30522, 0), (30522, 50), (49408, 0)])
def test_top_p_flat_cases_sandwich(dev, V, top_k):
    """cut lies between the fp64 thresholds of top_p - DELTA and top_p + DELTA (DELTA: the kernel's mass error, derived at the top of
    this file from its fixed-point scheme: 3.8e-7 bounded by 1e-6), and kept == #{y >= cut} exactly"""
    from valor_amd import decode
    from test_sample_filter_cpu import FLAT_CASES, flat_row
    row = flat_row(V)
    logits = padded(row[None].repeat(2, 1), dev)
    for inv, p, size in FLAT_CASES:
        pf = f32(p)                                         # the kernel's top_p is an fp32 value
        y = row * torch.tensor(inv, dtype=torch.float32)
        res = fdraw(logits, 8, 3, inv, top_k, pf)
        n_lo, cut_hi = decode.filter_row(y, top_k, pf - DELTA)
        n_hi, cut_lo = decode.filter_row(y, top_k, pf + DELTA)
        kept, cut = int(res[3][0]), float(res[4][0])
        print(f"[flat V={V} k={top_k} inv={inv:.4f} p={p}] kept {kept} (fp64 {n_lo}..{n_hi}), cut {cut:.6f}")
        assert cut_lo <= cut <= cut_hi and n_lo <= kept <= n_hi, (kept, n_lo, n_hi, cut, cut_lo, cut_hi)
        assert res[3][1] == res[3][0] and res[4][1] == res[4][0]
        if V == 30522 and top_k == 0:
            assert abs(kept - size) <= 6
        if top_k:
            assert kept <= 50
        check_draw(logits, 8, 3, inv, res)


def test_filtered_distribution_and_determinism(dev):
    torch.manual_seed(0)
    row = torch.randn(16, dtype=torch.float64) * 1.5
    R = 16384
    logits = row.float()[None].repeat(R, 1).to(dev)
    inv = f32(1 / 1.3)
    tok, lp, unf, kept, cut = fdraw(logits, 1234, 0, inv, 5, 1.0, eos=5)
    y = (row.float() * torch.tensor(inv, dtype=torch.float32)).double()
    S = torch.topk(y, 5).indices
    assert (kept == 5).all() and float(cut[0]) == float(y[S].min())
    t = tok.cpu()
    assert np.isin(t.numpy(), S.numpy()).all()                                  # no column outside the kept set is ever drawn
    pS = torch.softmax(y[S], 0).numpy()
    obs = np.array([(t == int(c)).sum() for c in S])
    chi2 = float(((obs - R * pS) ** 2 / (R * pS)).sum())
    assert chi2 < CHI2_DF4_P1E3, (chi2, obs, R * pS)
    ref = (y - torch.logsumexp(y[S], 0))[t].numpy()
    assert np.abs(lp.cpu().double().numpy() - ref).max() < 1e-5
    assert torch.equal(unf.cpu(), t != 5)
    again = fdraw(logits, 1234, 0, inv, 5, 1.0, eos=5)
    assert torch.equal(tok, again[0]) and same_bits(lp, again[1]) and torch.equal(kept, again[3]) and same_bits(cut, again[4])
    other = fdraw(logits, 1234, R * 4, inv, 5, 1.0, eos=5)
    assert not torch.equal(tok, other[0])


# ------------------------------------------------------------------------------------------------ generation
def _model(dev, cross_attn_type=None, **opts):
    import dataclasses
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    if cross_attn_type is not None:
        spec = dataclasses.replace(spec, cross_attn_type=cross_attn_type)
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    m = VALOR({"dropout": 0.0, "drop_path_rate": 0.0, "max_generation_len": 10, **opts}, spec=spec, dtype=torch.float32, device=dev)
    m.load_state_dict(sd, strict=True)
    return m, spec


def _batch(spec, b=3, seed=6):
    from valor_amd import synth
    batch = synth.make_batch(spec, batch=b, frames=2, audio_slices=2, txt_len=16, seed=seed)
    batch["ids"] = [f"clip{i}" for i in range(b)]
    return batch


def _gen(m, batch, groups=("tva",), **kw):
    from valor_amd import decode
    return {k: v.cpu() for k, v in decode.generate_cap(m, batch, list(groups), mode="sample", **kw).items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype == torch.float32:
            assert same_bits(a[k], b[k]), k
        else:
            assert torch.equal(a[k], b[k]), k


def test_generate_default_equals_filters_off_equals_the_unfiltered_loop(dev):
    from valor_amd import decode, kernels as K
    m, spec = _model(dev)
    batch = _batch(spec)
    try:
        base = _gen(m, batch, ("tva", "tv"), seed=11)
        off = _gen(m, batch, ("tva", "tv"), seed=11, temperature=1, top_k=0, top_p=1)
        _same(base, off)
        # the parent's loop restated: one step, one valor_sample_tokens launch
        with torch.no_grad():
            m.eval()
            b, kv_layers, ranges = decode.encode_for_generation(m, batch, ["tva", "tv"])
            stream = decode.SampleStream(11).begin_call()
            sess = decode.session(m, b, 1, 0, 10, kv_layers)
            sess.begin_batch(kv_layers)
            for g, key in (("tv", "t_v"), ("tva", "t_va")):
                sess.begin_group(ranges[g], None)
                sents = torch.full((b, 10), EOS, dtype=torch.long, device=dev)
                lps = torch.zeros((b, 10), device=dev)
                unf = torch.ones(b, dtype=torch.bool, device=dev)
                tok = torch.empty(b, dtype=torch.long, device=dev)
                for t in range(10):
                    logits = sess.step(None if t == 0 else tok)
                    seed, o = stream.take(b, logits.shape[1])
                    K.sample_tokens(logits, seed, o, EOS, unf, tok, sents[:, t], lps[:, t])
                assert torch.equal(sents.cpu(), base["generated_sequences_" + key]) and same_bits(lps.cpu(), base["logprobs_" + key])
    finally:
        decode.release_sessions(m)


def test_generate_top_k_1_times_4_is_greedy(dev):
    from valor_amd import decode
    m, spec = _model(dev)
    batch = _batch(spec)
    try:
        greedy = decode.generate_cap(m, batch, ["tva", "tv"], mode="greedy")
        out = _gen(m, batch, ("tva", "tv"), seed=4, top_k=1, num_return_sequences=4)
        for key in ("t_va", "t_v"):
            seq, lp = out["generated_sequences_" + key], out["logprobs_" + key]
            assert seq.shape == (12, 10) and lp.shape == (12, 10)
            assert torch.equal(seq, greedy["generated_sequences_" + key].cpu().repeat_interleave(4, 0))
            assert (lp == 0).all()
    finally:
        decode.release_sessions(m)


def test_generate_several_sequences_graphs_rerun_path_and_kept_session(dev, monkeypatch):
    from valor_amd import decode
    m, spec = _model(dev)
    batch = _batch(spec)
    kw = dict(top_p=0.9, temperature=0.8, num_return_sequences=4)
    try:
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "1")
        a = _gen(m, batch, ("tva", "tv"), seed=9, **kw)
        for key in ("t_va", "t_v"):
            s, lp = a["generated_sequences_" + key], a["logprobs_" + key]
            assert s.shape == (12, 10) and lp.shape == (12, 10)
            for r in range(12):
                hit = (s[r] == EOS).nonzero()
                if hit.numel():
                    j = int(hit[0])
                    assert (s[r, j:] == EOS).all() and (lp[r, j + 1:] == 0).all()
            assert torch.isfinite(lp).all() and (lp <= 0).all()
            assert any(not torch.equal(s[i * 4], s[i * 4 + j]) for i in range(3) for j in range(1, 4))   # the rows of a clip draw apart
        _same(a, _gen(m, batch, ("tva", "tv"), seed=9, **kw))                      # the same seed again (graph replay by now)
        assert not torch.equal(a["generated_sequences_t_va"], _gen(m, batch, seed=10, **kw)["generated_sequences_t_va"])
        # a kept (captured) session under other filter settings, then the first ones again
        b_kept = _gen(m, batch, ("tva", "tv"), seed=9, top_k=7, temperature=1.5, num_return_sequences=4)
        _same(a, _gen(m, batch, ("tva", "tv"), seed=9, **kw))
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "0")
        decode.release_sessions(m)
        _same(a, _gen(m, batch, ("tva", "tv"), seed=9, **kw))                      # eager steps
        _same(b_kept, _gen(m, batch, ("tva", "tv"), seed=9, top_k=7, temperature=1.5, num_return_sequences=4))
        monkeypatch.setenv("VALOR_KV_CACHE", "0")
        decode.release_sessions(m)
        c = _gen(m, batch, ("tva", "tv"), seed=9, **kw)                            # the re-run path
        for key in ("t_va", "t_v"):
            assert torch.equal(a["generated_sequences_" + key], c["generated_sequences_" + key])
            assert float((a["logprobs_" + key] - c["logprobs_" + key]).abs().max()) < 1e-4
    finally:
        decode.release_sessions(m)


def test_generate_rerun_path_with_a_block_per_modality(dev):
    """num_return_sequences through the per-modality cross blocks (_BlockKV: always the re-run path)"""
    from valor_amd import decode
    m, spec = _model(dev, cross_attn_type="va_parallel")
    batch = _batch(spec)
    try:
        greedy = decode.generate_cap(m, batch, ["tva"], mode="greedy")["generated_sequences_t_va"].cpu()
        out = _gen(m, batch, seed=2, top_k=1, num_return_sequences=2)
        assert torch.equal(out["generated_sequences_t_va"], greedy.repeat_interleave(2, 0))
        assert (out["logprobs_t_va"] == 0).all()
    finally:
        decode.release_sessions(m)


def test_generate_uses_the_models_sample_options(dev):
    from valor_amd import decode
    m, spec = _model(dev)
    mo, _ = _model(dev, sample_top_k=4, sample_top_p=0.8, sample_temperature=0.6)
    batch = _batch(spec)
    try:
        want = _gen(m, batch, seed=13, top_k=4, top_p=0.8, temperature=0.6)
        _same(want, _gen(mo, batch, seed=13))
        _same(_gen(m, batch, seed=13), _gen(mo, batch, seed=13, top_k=0, top_p=1.0, temperature=1.0))   # the call's arguments win
        assert not torch.equal(want["logprobs_t_va"], _gen(m, batch, seed=13)["logprobs_t_va"])
    finally:
        decode.release_sessions(m)
        decode.release_sessions(mo)
