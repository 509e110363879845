"""Generation controls through the decode loops. Scripted steps first (a stub session / stub stepper that return prepared logits, so the
tests do not depend on what a random model happens to generate): greedy under no_repeat_ngram_size / min_length / suppress_tokens ==
the host law applied step by step, beam search == a test-local loop (host law + the existing beam_select), length_penalty at the final
pick. Then the small synthetic model: controls off == the plain call bit for bit, cached == re-run path, graphs on == off, a kept session
under two settings, the properties on every output row, the sampled decode == host law + valor_sample_tokens_filtered bit for bit,
generate_qa(mode='sample'), the model's generation_* options through generate_cap and validate_cap."""
import math
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

EOS = 102
INF = float("inf")
B, V, L, SEP = 3, 40, 8, 2                  # the scripted geometry; its [SEP] is column 2 (decode.EOS is patched: 102 is no column of 40)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ scripted steps
class StubSession:
    """what the loops use of a DecodeSession: .m.device, .poll and .step(tok, parent) -> this step's prepared logits [rows, V]"""
    poll = 8

    def __init__(self, script, dev):
        self.m = types.SimpleNamespace(device=dev)
        self.script = [s.to(dev) for s in script]
        self.t = 0
        self.toks = []

    def step(self, tok=None, parent=None):
        self.toks.append(None if tok is None else tok.clone())
        out = self.script[self.t].clone()
        self.t += 1
        return out


class StubStepper:
    """what the re-run source uses of a _Stepper: .m.device, .b and .logits(state, rows); the rows are beam-major like the script's and
    the session's. Keeps the states it was handed."""

    def __init__(self, script, dev, b):
        self.m = types.SimpleNamespace(device=dev)
        self.script = [s.to(dev) for s in script]
        self.b = b
        self.states = []

    def logits(self, state, rows):
        self.states.append(None if state is None else state.clone())
        assert state is None or (state.shape[0] == rows and state.dtype == torch.int64 and state.device.type == "cpu")
        t = 0 if state is None else state.shape[1]
        return self.script[t][:rows].clone()


def rerun_source(script, dev):
    """the re-run step source over the script: its host-state bookkeeping runs, the decoder is the stub"""
    from valor_amd import decode
    return decode._Rerun(StubStepper(script, dev, B))


@pytest.fixture
def sep(monkeypatch):
    from valor_amd import decode
    monkeypatch.setattr(decode, "EOS", SEP)
    return SEP


def alternating_script():
    """greedy without controls: 7 8 7 8 ...; every row has its own order of runners-up"""
    g = torch.Generator().manual_seed(0)
    script = []
    for t in range(L):
        z = torch.randn((B, V), generator=g)
        z[:, SEP] = -6.0
        z[:, 7] = 9.0 if t % 2 == 0 else 8.0
        z[:, 8] = 8.0 if t % 2 == 0 else 9.0
        z[:, 9] = 7.0
        script.append(z)
    return script


def host_greedy(script, c, eos):
    """decode_greedy's bookkeeping with the host law in the place of the launch"""
    from valor_amd import decode
    sents = torch.full((B, L), eos, dtype=torch.long)
    unfinished = torch.ones(B, dtype=torch.bool)
    for t in range(L):
        z = decode.constrain_rows_host(script[t], sents, t, c, eos, unfinished)
        wt = z.argmax(1)
        unfinished = unfinished & (wt != eos)
        sents[:, t] = torch.where(unfinished, wt, torch.full_like(wt, eos))
    return sents


def repeated_ngrams(row, n, eos):
    row = row.tolist()
    if eos in row:
        row = row[:row.index(eos)]
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(grams) - len(set(grams))


def both_greedy(script, dev, c):
    from valor_amd import decode
    a = decode.decode_greedy(StubSession(script, dev), B, L, c)[0].cpu()
    b = decode.decode_greedy(rerun_source(script, dev), B, L, c)[0].cpu()
    assert torch.equal(a, b)
    return a


def test_scripted_greedy_no_repeat_ngram(dev, sep):
    from valor_amd import decode
    script = alternating_script()
    plain = both_greedy(script, dev, None)
    assert torch.equal(plain, torch.tensor([7, 8] * (L // 2)).repeat(B, 1))                      # the condition of the test
    assert torch.equal(both_greedy(script, dev, decode.Constraints()), plain)
    c = decode.Constraints(no_repeat_ngram_size=2)
    got = both_greedy(script, dev, c)
    assert torch.equal(got, host_greedy(script, c, sep))
    assert got[:, :3].tolist() == [[7, 8, 7]] * B and (got[:, 3] != 8).all()
    assert all(repeated_ngrams(r, 2, sep) == 0 for r in got)
    c = decode.Constraints(no_repeat_ngram_size=3, repetition_penalty=1.3)
    got = both_greedy(script, dev, c)
    assert torch.equal(got, host_greedy(script, c, sep)) and all(repeated_ngrams(r, 3, sep) == 0 for r in got)


def test_scripted_greedy_min_length_and_suppress(dev, sep):
    from valor_amd import decode
    script = alternating_script()
    for z in script:
        z[:, sep] = 20.0                                                                         # [SEP] wins every step
    assert (both_greedy(script, dev, None) == sep).all()
    c = decode.Constraints(min_length=4)
    got = both_greedy(script, dev, c)
    assert torch.equal(got, host_greedy(script, c, sep))
    assert (got[:, :4] != sep).all() and (got[:, 4:] == sep).all()
    script = alternating_script()
    c = decode.Constraints(suppress_tokens=(7, 7, 99, -3))
    got = both_greedy(script, dev, c)
    assert torch.equal(got, host_greedy(script, c, sep)) and not (got == 7).any() and (got[:, 0] == 8).all()


def local_beam(script, dev, beam, c, eos):
    """decode_beam's loop with the launch replaced: the device logits go to the host law and come back for the existing
    beam_select; rows beam-major, the history of row k * b + s = the words of beam k of sample s"""
    from valor_amd import decode
    seq_logprob = torch.zeros((B, 1, 1), device=dev)
    seq_mask = torch.ones((B, beam, 1), device=dev)
    outputs = torch.zeros((B, beam, L), dtype=torch.int64, device=dev)
    base = torch.arange(B, device=dev)
    selected = None
    for t in range(L):
        cur = 1 if t == 0 else beam
        logits = script[t].to(dev)[:B * cur]
        if t > 0:
            seq_mask = seq_mask * (selected.view(B, cur) != eos).float().unsqueeze(-1)
        hist = outputs.transpose(0, 1).reshape(B * beam, L).cpu()
        active = None if t == 0 else (seq_mask.view(B, beam).t().reshape(-1) != 0).cpu()
        logits = decode.constrain_rows_host(logits, hist, t, c, eos, active).to(dev)
        val, idx = decode.beam_select(logits, B, cur, beam, seq_logprob, seq_mask, beam_major=True, lse="xent")
        sel_beam = idx // V
        selected = idx - sel_beam * V
        seq_logprob = val.unsqueeze(-1)
        seq_mask = torch.gather(seq_mask, 1, sel_beam.unsqueeze(-1))
        if t > 0:
            outputs = torch.gather(outputs, 1, sel_beam.unsqueeze(-1).expand(B, beam, L))
        outputs[:, :, t] = selected
    order = torch.sort(seq_logprob, 1, descending=True)[1]
    return torch.gather(outputs, 1, order.expand(B, beam, L))[:, 0].cpu()


def cut(seqs, eos):
    return [r[:r.index(eos) + 1] if eos in r else r for r in seqs.tolist()]


def test_scripted_beam_equals_host_law_plus_beam_select(dev, sep):
    from valor_amd import decode
    beam = 3
    g = torch.Generator().manual_seed(1)
    script = []
    for t in range(L):
        z = torch.randn((B * beam, V), generator=g) * 0.5
        z[:, 7] += 4.0 if t % 2 == 0 else 3.0
        z[:, 8] += 3.0 if t % 2 == 0 else 4.0
        z[:, sep] += 2.5 if t >= 4 else -4.0
        script.append(z)
    plain = decode.decode_beam(StubSession(script, dev), B, beam, L).cpu()
    assert torch.equal(plain, local_beam(script, dev, beam, decode.Constraints(), sep))
    assert any(repeated_ngrams(r, 2, sep) > 0 for r in plain)                                    # the condition: the plain search repeats
    for c in (decode.Constraints(no_repeat_ngram_size=2), decode.Constraints(no_repeat_ngram_size=2, min_length=6, suppress_tokens=(9, 7)),
              decode.Constraints(no_repeat_ngram_size=3, repetition_penalty=1.3), decode.Constraints(no_repeat_ngram_size=1)):
        want = local_beam(script, dev, beam, c, sep)
        got = decode.decode_beam(StubSession(script, dev), B, beam, L, c).cpu()
        assert torch.equal(got, want), c
        rerun = decode.decode_beam(rerun_source(script, dev), B, beam, L, c).cpu()
        assert torch.equal(rerun, want), c                                                        # one loop, one selection: the ties behind [SEP] too
        n = c.no_repeat_ngram_size
        assert all(repeated_ngrams(r, n, sep) == 0 for r in got) and not torch.equal(got, plain)
    got = decode.decode_beam(StubSession(script, dev), B, beam, L, decode.Constraints(min_length=6, suppress_tokens=(9, 7))).cpu()
    assert all(len(r) >= 6 for r in cut(got, sep)) and not (got == 7).any() and not (got == 9).any()


def length_script():
    """beam 3, the same for every sample. Step 0: 10 (p .5), 11 (.4), 12 (.1). Step 1: after 10, [SEP] (.6) or 20 (.4); after 11, 21;
    after 12, 22. [11 21] (.4) leads, [10 SEP] (.3) has ended -- its score stands for every word, so its copies take the other two
    beams (the reference's rule). The leader goes on 22 23 24 25 26 with p 1 and ends at the last step with [SEP] (p .9): logP ln .36,
    8 tokens, against ln .3, 2 tokens."""
    beam = 3
    lo = -40.0
    script = []
    for t in range(L):
        z = torch.full((beam, V), lo)
        if t == 0:
            z[:, 10], z[:, 11], z[:, 12] = math.log(.5), math.log(.4), math.log(.1)
        elif t == 1:
            z[0, SEP], z[0, 20] = math.log(.6), math.log(.4)
            z[1, 21] = 0.0
            z[2, 22] = 0.0
        elif t < L - 1:
            z[:, 20 + t] = 0.0
        else:
            z[:, SEP], z[:, 39] = math.log(.9), math.log(.1)
        script.append(z.repeat_interleave(B, 0))                                                  # beam-major rows k * B + s
    return script


def test_scripted_length_penalty_at_the_final_pick(dev, sep):
    from valor_amd import decode
    script = length_script()
    long_h, short_h = [11, 21, 22, 23, 24, 25, 26, sep], [10, sep]
    # the formula: logP / len^alpha
    score = lambda p, n, a: math.log(p) / n ** a
    assert score(.36, 8, 0.0) > score(.3, 2, 0.0) and score(.36, 8, 1.0) > score(.3, 2, 1.0) and score(.36, 8, -1.0) < score(.3, 2, -1.0)
    for alpha, want in ((None, long_h), (0.0, long_h), (1.0, long_h), (-1.0, short_h)):
        c = None if alpha is None else decode.Constraints(length_penalty=alpha)
        got = decode.decode_beam(StubSession(script, dev), B, 3, L, c).cpu()
        assert cut(got, sep) == [want] * B, (alpha, got)
        got = decode.decode_beam(rerun_source(script, dev), B, 3, L, c).cpu()
        assert cut(got, sep) == [want] * B, (alpha, got)


def test_rerun_source_reorders_its_host_state_by_parent(dev):
    """decode._Rerun driven like decode_beam drives a source: the state the stepper is handed at step t == the words so far of a
    [b, beam, L] history gathered along the chosen beams, read beam-major. The chosen beams are fixed, never the identity for a whole
    step, and twice rows of a sample share a parent (once all three)."""
    from valor_amd import decode
    beam, R = 3, B * 3
    gen = torch.Generator().manual_seed(7)
    script = [torch.randn((R, V), generator=gen) for _ in range(L)]
    stub = StubStepper(script, dev, B)
    src = decode._Rerun(stub)
    assert src.poll == 1 and src.m is stub.m
    picks = ([1, 0, 2], [2, 0, 1], [0, 0, 1], [2, 1, 0], [1, 1, 1], [0, 2, 1])
    words = torch.randint(3, V, (L - 1, B, beam), generator=gen)
    base = torch.arange(B)
    outputs = torch.zeros((B, beam, L), dtype=torch.int64)
    z = src.step()
    assert stub.states == [None] and same_bits(z.cpu(), script[0][:B])                            # the first step: b rows of [CLS]
    for t in range(1, L):
        # selection t - 1, as in decode_beam: the first one continues the single row of every sample
        sel_beam = torch.zeros((B, beam), dtype=torch.long) if t == 1 else torch.tensor([picks[(t + s) % len(picks)] for s in range(B)])
        if t > 1:
            outputs = torch.gather(outputs, 1, sel_beam.unsqueeze(-1).expand(B, beam, L))
        outputs[:, :, t - 1] = words[t - 1]
        parent = (sel_beam.t() * B + base[None]).reshape(-1)
        assert t == 1 or not torch.equal(parent, torch.arange(R))
        z = src.step(words[t - 1].t().reshape(-1).to(dev), parent.to(dev))
        want = outputs.transpose(0, 1).reshape(R, L)[:, :t]                                      # row k * B + s: the words of beam k of sample s
        assert torch.equal(stub.states[t], want), t
        assert same_bits(z.cpu(), script[t])
    assert len(stub.states) == L
    # without `parent` (greedy, sampling) the rows stay where they are
    stub = StubStepper(script, dev, B)
    src = decode._Rerun(stub)
    src.step()
    for t in range(1, 4):
        src.step(words[t - 1, :, 0].to(dev))
    assert torch.equal(stub.states[3], words[:3, :, 0].t())


# ------------------------------------------------------------------------------------------------ the small synthetic model
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


def _batch(spec, b=3, seed=6, questions=False):
    from valor_amd import synth
    batch = synth.make_batch(spec, batch=b, frames=2, audio_slices=2, txt_len=16, seed=seed, questions=questions)
    batch["ids"] = [f"clip{i}" for i in range(b)]
    return batch


def _cap(m, batch, groups=("tva", "tv"), **kw):
    from valor_amd import decode
    return {k: v.cpu() for k, v in decode.generate_cap(m, batch, list(groups), **kw).items()}


def _qa(m, batch, groups=("tva", "tv"), **kw):
    from valor_amd import decode
    prompt = m.qa_prompt(batch["question_tokens"]["bert_tokens"].cpu())
    return {k: v.cpu() for k, v in decode.generate_qa(m, batch, list(groups), prompt, **kw).items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype == torch.float32:
            assert same_bits(a[k], b[k]), k
        else:
            assert torch.equal(a[k], b[k]), k


def _same_tokens(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype != torch.float32:
            assert torch.equal(a[k], b[k]), k


OFF = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=(), length_penalty=0.0)
MODES = (dict(mode="greedy"), dict(beam_size=3), dict(mode="sample", seed=5, top_k=20, temperature=0.9))


def check_rows(seqs, n=0, min_length=0, suppress=()):
    for row in seqs:
        assert repeated_ngrams(row, n, EOS) == 0 if n else True, row
        r = row.tolist()
        assert (r.index(EOS) if EOS in r else len(r)) >= min_length, row
        assert not set(r) & set(suppress), row


def test_controls_off_are_the_plain_call_bit_for_bit(dev):
    from valor_amd import decode
    m, spec = _model(dev)
    batch, qb = _batch(spec), _batch(spec, questions=True)
    try:
        for kw in MODES:
            _same(_cap(m, batch, **kw), _cap(m, batch, **kw, **OFF))
            _same(_qa(m, qb, **kw), _qa(m, qb, **kw, **OFF))
        # the loops themselves: no constraints == Constraints()
        with torch.no_grad():
            m.eval()
            b, kv_layers, ranges = decode.encode_for_generation(m, batch, ["tva"])
            for beam in (1, 3):
                a = decode._decode_groups(m, ["tva"], b, kv_layers, ranges, "caption", beam, 10)["tva"][0]
                c = decode._decode_groups(m, ["tva"], b, kv_layers, ranges, "caption", beam, 10, constraints=decode.Constraints())["tva"][0]
                assert torch.equal(a, c)
    finally:
        decode.release_sessions(m)


def test_controls_on_cached_rerun_graphs_and_a_kept_session(dev, monkeypatch):
    from valor_amd import decode
    m, spec = _model(dev)
    batch, qb = _batch(spec), _batch(spec, questions=True)
    try:
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "1")
        first = int(_cap(m, batch, mode="greedy")["generated_sequences_t_va"][0, 0])
        assert first != EOS
        one = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_length=5, suppress_tokens=(first, 100, 103, 0))
        two = dict(no_repeat_ngram_size=3, min_length=8, length_penalty=1.0)
        res = {}
        for name, ctl in (("one", one), ("two", two), ("one_again", one)):            # a kept session serves two settings in a row
            for i, kw in enumerate(MODES):
                res[name, "cap", i] = _cap(m, batch, **kw, **ctl)
                res[name, "qa", i] = _qa(m, qb, **kw, **ctl)
        for what in ("cap", "qa"):
            for i in range(len(MODES)):
                _same(res["one", what, i], res["one_again", what, i])
                out = res["one", what, i]
                for k, v in out.items():
                    if v.dtype != torch.float32:
                        check_rows(v, 2, 5, (first, 100, 103, 0))
                for k, v in res["two", what, i].items():
                    if v.dtype != torch.float32:
                        check_rows(v, 3, 8)
        assert not torch.equal(res["one", "cap", 0]["generated_sequences_t_va"], _cap(m, batch, mode="greedy")["generated_sequences_t_va"])
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "0")
        decode.release_sessions(m)
        for i, kw in enumerate(MODES):                                                # eager steps
            _same(res["one", "cap", i], _cap(m, batch, **kw, **one))
            _same(res["two", "qa", i], _qa(m, qb, **kw, **two))
        monkeypatch.setenv("VALOR_KV_CACHE", "0")
        decode.release_sessions(m)
        for i, kw in enumerate(MODES):                                                # the re-run path: token for token
            _same_tokens(res["one", "cap", i], _cap(m, batch, **kw, **one))
            _same_tokens(res["one", "qa", i], _qa(m, qb, **kw, **one))
            _same_tokens(res["two", "cap", i], _cap(m, batch, **kw, **two))
    finally:
        decode.release_sessions(m)


def test_rerun_path_with_a_block_per_modality_equals_a_host_law_loop(dev):
    """cross_attn_type 'va_parallel' always takes the re-run path (_Stepper): greedy under controls == the stepper's logits through the
    host law, step by step"""
    from valor_amd import decode
    m, spec = _model(dev, cross_attn_type="va_parallel")
    batch = _batch(spec)
    ctl = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_length=5, suppress_tokens=(100, 103))
    c = decode.Constraints(**ctl)
    try:
        got = _cap(m, batch, ("tva",), mode="greedy", **ctl)["generated_sequences_t_va"]
        check_rows(got, 2, 5, (100, 103))
        with torch.no_grad():
            m.eval()
            b, kv_layers, ranges = decode.encode_for_generation(m, batch, ["tva"])
            step = decode.stepper(m, "tva", b, kv_layers, ranges)
            sents = torch.full((b, 10), EOS, dtype=torch.long)
            unfinished = torch.ones(b, dtype=torch.bool)
            for t in range(10):
                z = decode.constrain_rows_host(step.logits(sents[:, :t] if t else None, b), sents, t, c, EOS, unfinished)
                wt = z.argmax(1)
                unfinished = unfinished & (wt != EOS)
                sents[:, t] = torch.where(unfinished, wt, torch.full_like(wt, EOS))
        assert torch.equal(got, sents)
        for kw in MODES[1:]:
            out = _cap(m, batch, ("tva",), **kw, **ctl)["generated_sequences_t_va"]
            check_rows(out, 2, 5, (100, 103))
    finally:
        decode.release_sessions(m)


def test_lm_greedy_is_the_same_through_both_sources(dev):
    """caption_type 'lm' (one new row per step, no [MASK]): decode_greedy over the session and over the re-run source, token for token"""
    from valor_amd import decode
    m, spec = _model(dev, caption_type="lm")
    batch = _batch(spec)
    c = decode.Constraints(no_repeat_ngram_size=2, min_length=4)
    try:
        with torch.no_grad():
            m.eval()
            b, kv_layers, ranges = decode.encode_for_generation(m, batch, ["tva"])
            sess = decode.session(m, b, 1, 0, 10, kv_layers)
            assert sess.J == 1 and sess.poll == 8
            sess.begin_batch(kv_layers)
            for con in (None, c):
                sess.begin_group(ranges["tva"], None)
                cached = decode.decode_greedy(sess, b, 10, con)[0].cpu()
                rerun = decode.decode_greedy(decode._Rerun(decode.stepper(m, "tva", b, kv_layers, ranges)), b, 10, con)[0].cpu()
                assert torch.equal(cached, rerun), (con, cached, rerun)
            check_rows(cached, 2, 4)
    finally:
        decode.release_sessions(m)


def test_sampled_decode_equals_host_law_plus_the_filtered_sampler(dev):
    from valor_amd import decode, kernels as K
    m, spec = _model(dev)
    batch = _batch(spec)
    ctl = dict(no_repeat_ngram_size=2, repetition_penalty=1.3, min_length=4, suppress_tokens=(100, 103))
    c = decode.Constraints(**ctl)
    smp = decode.Sampling(temperature=0.8, top_k=30, top_p=0.95)
    try:
        got = _cap(m, batch, ("tva", "tv"), mode="sample", seed=11, temperature=0.8, top_k=30, top_p=0.95, **ctl)
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
                    z = decode.constrain_rows_host(logits, sents.cpu(), t, c, EOS, unf.cpu()).to(dev)
                    seed, o = stream.take(b, z.shape[1])
                    K.sample_tokens_filtered(z, seed, o, EOS, unf, tok, sents[:, t], lps[:, t], smp.inv_temperature, smp.top_k, smp.top_p)
                assert torch.equal(sents.cpu(), got["generated_sequences_" + key]) and same_bits(lps.cpu(), got["logprobs_" + key]), key
                check_rows(sents.cpu(), 2, 4, (100, 103))
                assert torch.isfinite(lps).all() and (lps <= 0).all()
    finally:
        decode.release_sessions(m)


def test_generate_qa_sample_mode(dev):
    from valor_amd import decode, synth
    m, spec = _model(dev)
    qb = _batch(spec, questions=True)
    try:
        a = _qa(m, qb, mode="sample", seed=3, temperature=1.5)
        assert set(a) == {"generated_answers_t_va", "generated_answers_t_v", "logprobs_t_va", "logprobs_t_v"}
        assert a["generated_answers_t_va"].shape == (3, 10) and a["logprobs_t_va"].shape == (3, 10)
        _same(a, _qa(m, qb, mode="sample", seed=3, temperature=1.5))                    # deterministic per seed
        assert not torch.equal(a["generated_answers_t_va"], _qa(m, qb, mode="sample", seed=4, temperature=1.5)["generated_answers_t_va"])
        greedy = _qa(m, qb, mode="greedy")
        assert set(greedy) == {"generated_answers_t_va", "generated_answers_t_v"}
        _same(greedy, _qa(m, qb))                                                       # beam_size_qa 1: the default is greedy
        k1 = _qa(m, qb, mode="sample", seed=9, top_k=1)
        for key in ("t_va", "t_v"):
            assert torch.equal(k1["generated_answers_" + key], greedy["generated_answers_" + key]) and (k1["logprobs_" + key] == 0).all()
        # several questions per clip
        four = synth.make_batch(spec, batch=4, frames=2, audio_slices=2, txt_len=16, seed=9, questions=True)
        sq = dict(qb, question_tokens=four["question_tokens"], sample_num=[2, 1, 1])
        s = _qa(m, sq, mode="sample", seed=3, top_k=1, no_repeat_ngram_size=2)
        g = _qa(m, sq, mode="greedy", no_repeat_ngram_size=2)
        assert s["generated_answers_t_va"].shape == (4, 10)
        for key in ("t_va", "t_v"):
            assert torch.equal(s["generated_answers_" + key], g["generated_answers_" + key])
            check_rows(s["generated_answers_" + key], 2)
        _same(_qa(m, sq, mode="sample", seed=6, top_p=0.9), _qa(m, sq, mode="sample", seed=6, top_p=0.9))
    finally:
        decode.release_sessions(m)


def test_model_options_are_the_defaults_and_reach_validate_cap(dev, tmp_path):
    import json
    from valor_amd import decode
    from valor_amd.evaluate import validate_cap
    ctl = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_length=5, suppress_tokens=(100, 103), length_penalty=0.5)
    m, spec = _model(dev)
    mo, _ = _model(dev, **{"generation_" + k: v for k, v in ctl.items()})
    batch = _batch(spec)
    try:
        for kw in MODES:
            want = _cap(m, batch, **kw, **ctl)
            _same(want, _cap(mo, batch, **kw))
            _same(_cap(m, batch, **kw), _cap(mo, batch, **kw, **OFF))                  # the call's arguments win
        plain = _cap(m, batch, mode="greedy")
        assert not torch.equal(plain["generated_sequences_t_va"], _cap(mo, batch, mode="greedy")["generated_sequences_t_va"])
        # validate_cap goes through the model's forward: the options are all it has
        seen = []

        def dec(seqs):
            seen.append(seqs.cpu())
            return [" ".join(f"w{int(x)}" for x in (r[:r.index(EOS)] if EOS in r else r)) or "w0" for r in seqs.tolist()]
        refs = {i: ["w1 w2 w3"] for i in batch["ids"]}
        for beam in (1, 3):
            mo.beam_size = beam
            log = validate_cap(mo, [batch], "cap%tva%tv", refs, decode=dec, scorer="host", output_dir=str(tmp_path), global_step=beam)
            assert set(log) == {"tva", "tv"}
            out = json.load(open(tmp_path / "results_test_" / f"step_{beam}_tva.json"))
            for r in out:
                ids = torch.tensor([int(w[1:]) for w in r["caption"].split()] + [EOS])
                check_rows(ids[None], 2, 5, (100, 103))
        assert len(seen) == 4
        for s in seen:
            check_rows(s, 2, 5, (100, 103))
    finally:
        decode.release_sessions(m)
        decode.release_sessions(mo)
