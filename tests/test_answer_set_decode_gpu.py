"""Closed answer sets through the decode loops. Scripted steps first (a stub session / stub stepper that return prepared logits): greedy,
beam-3 and sampled decoding inside a set == a host loop built from decode.trie_rows_host and the unchanged selection, token for token;
one candidate per sample under beam 3 (fewer live continuations than beams at every step: the case a -inf mask cannot serve); every
sampled draw inside the set. Then the small synthetic fp32 model: every route (cached + graph, a kept session, eager steps, the re-run
path) answers inside the set and the routes agree; candidates=None is the plain call; score_candidates against teacher-forced fp64
log-softmax sums of the re-run stepper; an exhaustive beam search picks the best-scored candidate; validate_qa in both new modes with
planted answers; one bf16 run."""
import json
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
B, V, L, SEP = 3, 40, 8, 2                  # the scripted geometry; its [SEP] is column 2 (decode.EOS is patched: 102 is no column of 40)
TERM = 5e-5                                 # per term of a score, cached session against the re-run path: twice the 2e-5 logit band of
#                                             tests/test_decode_cache_gpu.py:102 plus its 1e-5 log-sum-exp band (:193)


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

    def step(self, tok=None, parent=None):
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


def script_of(seed, rows=B * 3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((rows, V), generator=g) * 2.0 for _ in range(L)]


def scripted_sets():
    from valor_amd import decode
    shared = decode.AnswerSet([[7, 8, 9], [7, 8], [7, 5], [30], [10, 11, 12, 13], [7, 8]])
    per = decode.AnswerSet([[[7, 8, 9], [7, 8], [30]], [[10, 11, 12, 13, 14, 15]], [[5], [6, 5], [6, 6, 6]]], per_sample=True)
    one = decode.AnswerSet([[[7, 8, 9]], [[30]], [[10, 11, 12, 13, 14, 15]]], per_sample=True)
    return shared, per, one


def host_greedy(script, a, eos):
    """decode_greedy's bookkeeping with the host law in the place of the launch"""
    from valor_amd import decode
    sents = torch.full((B, L), eos, dtype=torch.long)
    unfinished = torch.ones(B, dtype=torch.bool)
    for t in range(L):
        z = decode.trie_rows_host(script[t][:B], sents, t, a, eos, B, unfinished)
        wt = z.argmax(1)
        unfinished = unfinished & (wt != eos)
        sents[:, t] = torch.where(unfinished, wt, torch.full_like(wt, eos))
    return sents


def test_scripted_greedy_equals_the_host_law_loop(dev, sep):
    from valor_amd import decode
    for seed in (0, 1):
        script = script_of(seed, rows=B)
        plain = decode.decode_greedy(StubSession(script, dev), B, L)[0].cpu()
        for a in scripted_sets():
            want = host_greedy(script, a, sep)
            got = decode.decode_greedy(StubSession(script, dev), B, L, None, a)[0].cpu()
            rerun = decode.decode_greedy(rerun_source(script, dev), B, L, None, a)[0].cpu()
            assert torch.equal(got, want) and torch.equal(rerun, want), (seed, got, want)
            assert (a.index_of(got) >= 0).all() and not torch.equal(got, plain)
    # length_penalty is no logits rule: it may stay; a logits rule may not
    a = scripted_sets()[0]
    decode.decode_greedy(StubSession(script, dev), B, L, decode.Constraints(length_penalty=1.0), a)
    with pytest.raises(ValueError, match="candidates"):
        decode.decode_greedy(StubSession(script, dev), B, L, decode.Constraints(min_length=2), a)


def local_beam(script, dev, beam, a, eos):
    """decode_beam's loop with the launch replaced: the device logits go to the host law and come back for the existing
    beam_select (which is given the log-sum-exp of the rows before the mask: a hypothesis' score is the model's sequence logP); rows
    beam-major, the history of row k * b + s = the words of beam k of sample s. -> (best sequences, their logP)"""
    from valor_amd import decode
    seq_logprob = torch.zeros((B, 1, 1), device=dev)
    seq_mask = torch.ones((B, beam, 1), device=dev)
    outputs = torch.zeros((B, beam, L), dtype=torch.int64, device=dev)
    selected = None
    for t in range(L):
        cur = 1 if t == 0 else beam
        logits = script[t].to(dev)[:B * cur]
        if t > 0:
            seq_mask = seq_mask * (selected.view(B, cur) != eos).float().unsqueeze(-1)
        hist = outputs.transpose(0, 1).reshape(B * beam, L).cpu()
        active = None if t == 0 else (seq_mask.view(B, beam).t().reshape(-1) != 0).cpu()
        lse = decode.row_lse(logits)[0]
        logits = decode.trie_rows_host(logits, hist, t, a, eos, B, active).to(dev)
        val, idx = decode.beam_select(logits, B, cur, beam, seq_logprob, seq_mask, beam_major=True, lse="xent", lse_rows=lse)
        assert torch.isfinite(val).all(), t                                                      # no NaN, no -inf: the floor is finite
        sel_beam = idx // V
        assert ((sel_beam >= 0) & (sel_beam < cur)).all(), t                                     # every beam got a candidate: no sentinel
        selected = idx - sel_beam * V
        seq_logprob = val.unsqueeze(-1)
        seq_mask = torch.gather(seq_mask, 1, sel_beam.unsqueeze(-1))
        if t > 0:
            outputs = torch.gather(outputs, 1, sel_beam.unsqueeze(-1).expand(B, beam, L))
        outputs[:, :, t] = selected
    order = torch.sort(seq_logprob, 1, descending=True)[1]
    return torch.gather(outputs, 1, order.expand(B, beam, L))[:, 0].cpu(), torch.gather(seq_logprob, 1, order)[:, 0, 0].cpu()


def cut(seqs, eos):
    return [r[:r.index(eos) + 1] if eos in r else r for r in seqs.tolist()]


def test_scripted_beam_equals_host_law_plus_beam_select(dev, sep, monkeypatch):
    from valor_amd import decode
    beam = 3
    for seed in (2, 3):
        script = script_of(seed)
        for a in scripted_sets():
            want, logp = local_beam(script, dev, beam, a, sep)
            got = decode.decode_beam(StubSession(script, dev), B, beam, L, None, a).cpu()
            assert cut(got, sep) == cut(want, sep), (seed, got, want)
            assert (a.index_of(got) >= 0).all() and torch.isfinite(logp).all() and (logp > -1e3).all()
            rerun = decode.decode_beam(rerun_source(script, dev), B, beam, L, None, a).cpu()
            assert cut(rerun, sep) == cut(want, sep) and torch.equal(rerun, got), (seed, rerun, want)


def test_one_candidate_per_sample_under_beam_3(dev, sep, monkeypatch):
    """a single live continuation per sample at every step, three beams: the result is that candidate, its logP is finite, nothing is NaN,
    and the fused selection agrees with the reference's arithmetic (VALOR_BEAM_SELECT=0: 0/1 masks times the candidates)"""
    from valor_amd import decode
    one = scripted_sets()[2]
    script = script_of(4)
    want, logp = local_beam(script, dev, 3, one, sep)
    assert cut(want, sep) == [c[0] + [sep] for c in one.candidates]
    assert torch.isfinite(logp).all() and (logp > -1e3).all()
    # the law of the score: the sum of the step rows' log-softmax along the candidate (beam 0 carries it: rows s of every step)
    for s, (c,) in enumerate(one.candidates):
        ref = sum(float(torch.log_softmax(script[t][s].double(), 0)[w]) for t, w in enumerate(c + [sep]))
        assert abs(float(logp[s]) - ref) < 1e-4 * (len(c) + 1), (s, float(logp[s]), ref)
    for flag in ("1", "0"):
        monkeypatch.setenv("VALOR_BEAM_SELECT", flag)
        got = decode.decode_beam(StubSession(script, dev), B, 3, L, None, one).cpu()
        assert cut(got, sep) == cut(want, sep), flag
        rerun = decode.decode_beam(rerun_source(script, dev), B, 3, L, None, one).cpu()
        assert cut(rerun, sep) == cut(want, sep), flag


def host_sample(script, dev, a, eos, seed, sampling):
    """decode_sample's loop: the host law, then the unchanged sampler launch"""
    from valor_amd import decode, kernels as K
    stream = decode.SampleStream(seed).begin_call()
    sents = torch.full((B, L), eos, dtype=torch.long, device=dev)
    lps = torch.zeros((B, L), device=dev)
    unf = torch.ones(B, dtype=torch.bool, device=dev)
    tok = torch.empty(B, dtype=torch.long, device=dev)
    for t in range(L):
        z = decode.trie_rows_host(script[t][:B], sents.cpu(), t, a, eos, B, unf.cpu()).to(dev)
        sd, off = stream.take(B, V)
        if sampling is None:
            K.sample_tokens(z, sd, off, eos, unf, tok, sents[:, t], lps[:, t])
        else:
            K.sample_tokens_filtered(z, sd, off, eos, unf, tok, sents[:, t], lps[:, t], sampling.inv_temperature, sampling.top_k, sampling.top_p)
    return sents.cpu(), lps.cpu()


def test_scripted_sampling_equals_the_host_law_loop_and_stays_inside_the_set(dev, sep):
    from valor_amd import decode
    script = script_of(5, rows=B)
    seen = set()
    for a in scripted_sets():
        for sampling in (None, decode.Sampling(top_k=2, top_p=0.9), decode.Sampling(temperature=1.7)):
            for seed in range(6):
                want, want_lp = host_sample(script, dev, a, sep, seed, sampling)
                got, lp = decode.decode_sample(StubSession(script, dev), B, L, decode.SampleStream(seed).begin_call(), sampling, None, a)
                assert torch.equal(got.cpu(), want) and same_bits(lp.cpu(), want_lp), (seed, sampling)
                rr, rlp = decode.decode_sample(rerun_source(script, dev), B, L, decode.SampleStream(seed).begin_call(), sampling, None, a)
                assert torch.equal(rr.cpu(), want) and same_bits(rlp.cpu(), want_lp), (seed, sampling)
                idx = a.index_of(want)
                assert (idx >= 0).all(), (seed, sampling, want)                           # every draw lay in the allowed set
                assert torch.isfinite(want_lp).all() and (want_lp <= 0).all()
                seen.update((s, int(i)) for s, i in enumerate(idx))
    assert len(seen) > 3                                                                   # the draws do vary (three would be one answer per sample)


# ------------------------------------------------------------------------------------------------ the small synthetic model
def _model(dev, dtype=torch.float32, **opts):
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    m = VALOR({"dropout": 0.0, "drop_path_rate": 0.0, "max_generation_len": 10, **opts}, spec=spec, dtype=dtype, device=dev)
    m.load_state_dict(sd, strict=True)
    return m, spec


def _batch(spec, b=3, seed=6):
    from valor_amd import synth
    batch = synth.make_batch(spec, batch=b, frames=2, audio_slices=2, txt_len=16, seed=seed, questions=True)
    assert (batch["question_tokens"]["bert_tokens"] == 0).any()                             # zero-padded questions
    batch["ids"] = [f"clip{i}" for i in range(b)]
    return batch


def _qa(m, batch, groups=("tva", "tv"), **kw):
    from valor_amd import decode
    prompt = m.qa_prompt(batch["question_tokens"]["bert_tokens"].cpu())
    return {k: v.cpu() for k, v in decode.generate_qa(m, batch, list(groups), prompt, **kw).items()}


def _cap(m, batch, groups=("tva",), **kw):
    from valor_amd import decode
    return {k: v.cpu() for k, v in decode.generate_cap(m, batch, list(groups), **kw).items()}


def model_sets(spec):
    """a shared set of answers of 1..4 tokens with common prefixes, and a per-sample set of <= 3 answers with pairwise distinct first
    tokens (an exhaustive search under beam 3)"""
    from valor_amd import decode
    g = torch.Generator().manual_seed(11)
    w = torch.randint(200, spec.vocab, (40,), generator=g).tolist()
    shared = decode.AnswerSet([[w[0]], [w[0], w[1]], [w[0], w[1], w[2], w[3]], [w[4], w[5]], [w[6], w[7], w[8]], [w[9]], [w[4], w[10]]])
    per = decode.AnswerSet([[[w[11], w[12]], [w[13]], [w[14], w[15], w[16], w[17]]], [[w[18], w[19], w[20]], [w[21]]],
                            [[w[22]], [w[23], w[24]], [w[25], w[26], w[27]]]], per_sample=True)
    return shared, per


MODES = (dict(mode="greedy"), dict(beam_size=3), dict(mode="sample", seed=5), dict(mode="sample", seed=5, top_k=2, top_p=0.9))


def _tokens_equal(a, b):
    """the answers up to and including their [SEP] (behind it a beam's words are arbitrary ties)"""
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype != torch.float32:
            assert cut(a[k], EOS) == cut(b[k], EOS), k


def _same(a, b):
    _tokens_equal(a, b)
    for k in a:
        if a[k].dtype == torch.float32:
            assert same_bits(a[k], b[k]), k


def _inside(out, a):
    n = 0
    for k, v in out.items():
        if v.dtype != torch.float32:
            assert (a.index_of(v) >= 0).all(), (k, v)
            n += 1
        else:
            assert torch.isfinite(v).all() and (v <= 0).all(), k
    assert n


def test_every_route_answers_inside_the_set_and_the_routes_agree(dev, monkeypatch):
    from valor_amd import decode
    m, spec = _model(dev)
    qb, qb2 = _batch(spec), _batch(spec, seed=9)
    shared, per = model_sets(spec)
    try:
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "1")
        res = {}
        for name, a in (("shared", shared), ("per", per)):
            for i, kw in enumerate(MODES):
                res[name, i] = _qa(m, qb, **kw, candidates=a)                             # cached session, captured step
                _inside(res[name, i], a)
                _inside(_qa(m, qb2, **kw, candidates=a), a)                               # the kept session serves a second batch
                _same(res[name, i], _qa(m, qb, **kw, candidates=a))                       # ... and the first again, bit for bit
        plain = _qa(m, qb, mode="greedy")
        assert not torch.equal(plain["generated_answers_t_va"], res["shared", 0]["generated_answers_t_va"])
        assert (shared.index_of(plain["generated_answers_t_va"]) < 0).all()               # the condition: the free decoder leaves the set
        # a plain list of token lists is wrapped; captions take the argument too; forward_qa / forward_cap forward it
        _same(res["shared", 0], _qa(m, qb, mode="greedy", candidates=shared.candidates[0]))
        _inside(_cap(m, qb, mode="greedy", candidates=shared), shared)
        _inside(_cap(m, qb, mode="sample", seed=2, num_return_sequences=2, candidates=per), per.for_rows(6))
        fq = {k: v.cpu() for k, v in m.forward_qa(qb, "qa%tva%tv", compute_loss=False, candidates=per).items()}
        _same(fq, _qa(m, qb, candidates=per))
        _inside({k: v.cpu() for k, v in m.forward_cap(qb, "cap%tva", compute_loss=False, candidates=shared).items()}, shared)
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "0")
        decode.release_sessions(m)
        for name, a in (("shared", shared), ("per", per)):                                 # eager steps
            for i, kw in enumerate(MODES):
                _same(res[name, i], _qa(m, qb, **kw, candidates=a))
        monkeypatch.setenv("VALOR_KV_CACHE", "0")
        decode.release_sessions(m)
        for name, a in (("shared", shared), ("per", per)):                                 # the re-run path: token for token
            for i, kw in enumerate(MODES):
                out = _qa(m, qb, **kw, candidates=a)
                _tokens_equal(res[name, i], out)
                _inside(out, a)
    finally:
        decode.release_sessions(m)


def test_several_question_rows_per_clip(dev):
    """sample_num: a per-sample set with one entry per clip is read by all of the clip's question rows; one per question row is read as is"""
    from valor_amd import decode, synth
    m, spec = _model(dev)
    qb = _batch(spec)
    _, per = model_sets(spec)
    four = synth.make_batch(spec, batch=4, frames=2, audio_slices=2, txt_len=16, seed=9, questions=True)
    sq = dict(qb, question_tokens=four["question_tokens"], sample_num=[2, 1, 1])
    try:
        for kw in MODES[:2]:
            out = _qa(m, sq, **kw, candidates=per)["generated_answers_t_va"]
            assert out.shape[0] == 4 and (per.for_rows(4, [2, 1, 1]).index_of(out) >= 0).all()
            rows = per.with_roots([0, 0, 1, 2])
            assert torch.equal(out, _qa(m, sq, **kw, candidates=rows)["generated_answers_t_va"])
    finally:
        decode.release_sessions(m)


def test_candidates_none_is_the_plain_call_and_issues_no_launch(dev, monkeypatch):
    from valor_amd import decode, kernels as K
    m, spec = _model(dev)
    qb = _batch(spec)
    try:
        want = [(_qa(m, qb, **kw), _cap(m, qb, **kw)) for kw in MODES]

        def boom(*a, **k):
            raise AssertionError("valor_trie_constrain launched without candidates")
        monkeypatch.setattr(K, "trie_constrain", boom)
        def exact(x, y):
            assert x.keys() == y.keys() and all(same_bits(x[k], y[k]) if x[k].dtype == torch.float32 else torch.equal(x[k], y[k]) for k in x)
        for kw, (q, c) in zip(MODES, want):
            exact(q, _qa(m, qb, **kw, candidates=None))
            exact(c, _cap(m, qb, **kw, candidates=None))
        with pytest.raises(AssertionError, match="without candidates"):
            _qa(m, qb, mode="greedy", candidates=[[500]])
    finally:
        decode.release_sessions(m)


def reference_scores(m, batch, group, a, prompt):
    """teacher-forced on the re-run path: decode.stepper(...).logits, log-softmax and the sum in fp64 -> ([b, Cmax] fp64, lengths)"""
    from valor_amd import decode
    with torch.no_grad():
        m.eval()
        b, kv_layers, ranges = decode.encode_for_generation(m, batch, [group])
        step = decode.stepper(m, group, b, kv_layers, ranges, prompt)
        a = a.for_rows(b)
        per = [a.candidates[s % a.n_roots] for s in range(b)]
        Cmax = max(len(p) for p in per)
        out = torch.full((b, Cmax), -float("inf"), dtype=torch.float64)
        lens = torch.zeros((b, Cmax), dtype=torch.long)
        for j in range(Cmax):
            cands = [p[j] if j < len(p) else p[0] for p in per]
            T = max(len(c) for c in cands) + 1
            forced = torch.full((b, T), EOS, dtype=torch.long)
            for s, c in enumerate(cands):
                forced[s, :len(c)] = torch.tensor(c)
            score = torch.zeros(b, dtype=torch.float64)
            for t in range(T):
                lp = torch.log_softmax(step.logits(forced[:, :t] if t else None, b).double().cpu(), 1)
                for s, c in enumerate(cands):
                    if t <= len(c):
                        score[s] += lp[s, forced[s, t]]
            for s, p in enumerate(per):
                if j < len(p):
                    out[s, j], lens[s, j] = score[s], len(p[j])
    return out, lens


def test_score_candidates_against_the_rerun_path(dev):
    from valor_amd import decode
    m, spec = _model(dev)
    qb = _batch(spec)
    shared, per = model_sets(spec)
    prompt = m.qa_prompt(qb["question_tokens"]["bert_tokens"].cpu())
    try:
        decode.release_sessions(m)
        for a, max_rows, cmax in ((shared, 9, 7), (per, 3, 3), (shared, 512, 7)):          # 7 answers in chunks of 3: three chunks; 3 in chunks of 1
            got = decode.score_candidates(m, qb, ["tva", "tv"], a, prompt_cpu=prompt, max_rows=max_rows)
            assert set(got) == {"tva", "tv"} and not m.__dict__.get("_decode_sessions")      # the call left no session in the pool
            for g in ("tva", "tv"):
                sc = got[g]
                assert sc.is_cuda and sc.dtype == torch.float32 and tuple(sc.shape) == (3, cmax)
                ref, lens = reference_scores(m, qb, g, a, prompt)
                assert torch.equal(torch.isinf(sc.cpu()), torch.isinf(ref)) and not torch.isnan(sc).any()
                live = ~torch.isinf(ref)
                err = (sc.cpu().double() - ref)[live].abs()
                band = (lens[live] + 1).double() * TERM
                print(f"score_candidates {g} max_rows={max_rows}: max |err| {float(err.max()):.2e} (band per term {TERM})")
                assert (err <= band).all(), (g, max_rows, float((err / band).max()))
            if a is per:
                assert torch.isinf(got["tva"][1, 2]) and float(got["tva"][1, 2]) < 0            # sample 1 has two answers: its third slot is -inf
        # captions: no prompt rows
        got = decode.score_candidates(m, qb, ["tva"], shared, max_rows=9)["tva"].cpu().double()
        ref, lens = reference_scores(m, qb, "tva", shared, "caption")
        assert ((got - ref).abs() <= (lens + 1).double() * TERM).all()
    finally:
        decode.release_sessions(m)


def test_exhaustive_beam_search_picks_the_best_scored_candidate(dev):
    """<= 3 answers per sample with pairwise distinct first tokens under beam 3: every answer is searched, so the chosen one's exact score
    is the row's maximum (within the band of a score)"""
    from valor_amd import decode
    m, spec = _model(dev)
    shared, per = model_sets(spec)
    try:
        for seed in (6, 9):
            qb = _batch(spec, seed=seed)
            prompt = m.qa_prompt(qb["question_tokens"]["bert_tokens"].cpu())
            out = _qa(m, qb, beam_size=3, candidates=per)
            scores = decode.score_candidates(m, qb, ["tva", "tv"], per, prompt_cpu=prompt)
            for g, key in (("tva", "t_va"), ("tv", "t_v")):
                idx = per.index_of(out["generated_answers_" + key])
                assert (idx >= 0).all()
                sc = scores[g].cpu()
                chosen = sc.gather(1, idx[:, None])[:, 0]
                assert (chosen >= sc.max(1).values - (per.max_len + 1) * TERM).all(), (g, idx, sc)
    finally:
        decode.release_sessions(m)


# ------------------------------------------------------------------------------------------------ evaluation
RIGHT = [500, 501]


def plant(m):
    """the known answer: the decoder bias makes 500 the likeliest token, then 501, then [SEP] -- inside a set that holds [500 501] the
    constrained decoder says '500 501'; the free decoder repeats 500"""
    with torch.no_grad():
        bias = m.P["cls.decoder.bias"]
        bias[500] += 40.0
        bias[501] += 30.0
        bias[EOS] += 20.0


def dec(seqs):
    return [" ".join(str(int(x)) for x in (r[:r.index(EOS)] if EOS in r else r)) for r in seqs.tolist()]


def bert_rows(cands, T=8):
    rows = torch.zeros((len(cands), T), dtype=torch.long)
    for i, c in enumerate(cands):
        rows[i, 0], rows[i, 1:1 + len(c)], rows[i, 1 + len(c)] = 101, torch.tensor(c), EOS
    return rows


def loader_of(spec):
    """two batches of three questions, four choices each; the right one ([500 501]) sits at a different index for every question"""
    batches, gt = [], []
    for n, seed in enumerate((6, 9)):
        batch = _batch(spec, seed=seed)
        choices, answers = [], []
        for q in range(3):
            right = (q + 2 * n + 1) % 4
            wrong = [[500, 700 + q], [600 + 10 * n + q], [501, 640, 650 + q]]
            choices += wrong[:right] + [RIGHT] + wrong[right:]
            answers.append(right)
        batch["choice_tokens"] = {"bert_tokens": bert_rows(choices)}
        batch["answers"] = answers
        batch["question_ids"] = [f"q{n}_{q}" for q in range(3)]
        batches.append(batch)
        gt += answers
    return batches, gt


def test_validate_qa_multiple_choice(dev, tmp_path):
    from valor_amd import decode
    from valor_amd.evaluate import validate_qa
    m, spec = _model(dev)
    mo, _ = _model(dev, qa_multiple_choice=True)
    plant(m), plant(mo)
    loader, gt = loader_of(spec)
    try:
        log = validate_qa(m, loader, "qa%tva%tv", multiple_choice=True, output_dir=str(tmp_path), global_step=3, dset_name="mc")
        assert log == {"tv": {"accuracy": 100.0}, "tva": {"accuracy": 100.0}}
        folder = tmp_path / "predict_answers"
        assert json.load(open(folder / "step3_gt.json")) == gt and json.load(open(folder / "step3_tv_pred.json")) == gt      # indices
        sub = json.load(open(folder / "step3_tv_pred_submited_mc.json"))
        assert [r["question_id"] for r in sub] == [f"q{n}_{q}" for n in range(2) for q in range(3)] and [r["answer"] for r in sub] == gt
        assert not m.__dict__.get("_decode_sessions")
        # the integer answers in txt_tokens (the reference's collate), the option as the default
        alt = [dict({k: v for k, v in b.items() if k != "answers"}, txt_tokens=torch.tensor(b["answers"])) for b in loader]
        assert validate_qa(mo, alt, "qa%tv") == {"tv": {"accuracy": 100.0}}
        wrong = [dict(b, answers=[(a + 1) % 4 for a in b["answers"]]) for b in loader]
        assert validate_qa(m, wrong, "qa%tv", multiple_choice=True) == {"tv": {"accuracy": 0.0}}
        uneven = dict(loader[0], choice_tokens={"bert_tokens": loader[0]["choice_tokens"]["bert_tokens"][:11]})
        with pytest.raises(ValueError, match="same number of choices"):
            validate_qa(m, [uneven], "qa%tv", multiple_choice=True)
    finally:
        decode.release_sessions(m)
        decode.release_sessions(mo)


def test_validate_qa_inside_a_candidate_set(dev, tmp_path):
    from valor_amd import decode
    from valor_amd.evaluate import validate_qa
    cands = [[600], [500, 700], RIGHT, [501, 640, 650], RIGHT]
    m, spec = _model(dev)
    mo, _ = _model(dev, qa_answer_candidates=cands)
    plant(m), plant(mo)
    loader, _ = loader_of(spec)
    for b in loader:                                                                      # the training schema: '[CLS] answer [SEP]' rows
        b["txt_tokens"] = {"bert_tokens": bert_rows([RIGHT] * 3)}
        del b["answers"]
    try:
        for beam in (1, 3):
            m.beam_size = mo.beam_size = beam
            m.beam_size_qa = mo.beam_size_qa = beam
            assert validate_qa(m, loader, "qa%tva%tv", decode=dec)["tv"] == {"accuracy": 0.0}          # the free decoder: '500 500 500 ...'
            log = validate_qa(m, loader, "qa%tva%tv", decode=dec, candidates=decode.AnswerSet(cands), output_dir=str(tmp_path), global_step=beam)
            assert log == {"tv": {"accuracy": 100.0}, "tva": {"accuracy": 100.0}}
            folder = tmp_path / "predict_answers"
            assert json.load(open(folder / f"step{beam}_gt.json")) == ["500 501"] * 6
            assert json.load(open(folder / f"step{beam}_tv_pred.json")) == ["500 501"] * 6
            assert validate_qa(m, loader, "qa%tv", decode=dec, candidates=cands) == {"tv": {"accuracy": 100.0}}      # a plain list
            assert validate_qa(mo, loader, "qa%tv", decode=dec) == {"tv": {"accuracy": 100.0}}                       # the option is the default
    finally:
        decode.release_sessions(m)
        decode.release_sessions(mo)


def test_bf16_answers_inside_the_set_and_scores_within_the_logit_error(dev, monkeypatch):
    """bf16, the benchmarked arithmetic, at the same shape: every route answers inside the set, and the cached and the re-run scores agree
    within (L + 1) * 2 * BF16_LOGIT_BAND (both sides carry the bf16 logit error of a step)"""
    from test_finetune_gpu import BF16_LOGIT_BAND
    from valor_amd import decode
    m, spec = _model(dev, dtype=torch.bfloat16)
    qb = _batch(spec)
    shared, per = model_sets(spec)
    prompt = m.qa_prompt(qb["question_tokens"]["bert_tokens"].cpu())
    try:
        for a in (shared, per):
            for kw in MODES:
                _inside(_qa(m, qb, **kw, candidates=a), a)
        cached = {a: decode.score_candidates(m, qb, ["tva"], a, prompt_cpu=prompt, max_rows=9)["tva"].cpu() for a in (shared, per)}
        monkeypatch.setenv("VALOR_KV_CACHE", "0")
        decode.release_sessions(m)
        for a in (shared, per):
            for kw in MODES[:2]:
                _inside(_qa(m, qb, **kw, candidates=a), a)
            rerun = decode.score_candidates(m, qb, ["tva"], a, prompt_cpu=prompt, max_rows=9)["tva"].cpu()
            assert torch.equal(torch.isinf(rerun), torch.isinf(cached[a]))
            live = ~torch.isinf(rerun)
            lens = torch.tensor([[len(c) for c in p] + [0] * (rerun.shape[1] - len(p)) for p in
                                 [a.candidates[s % a.n_roots] for s in range(3)]])
            err = (rerun - cached[a])[live].abs()
            print(f"bf16 scores, cached against re-run: max |err| {float(err.max()):.4f}")
            assert (err <= (lens[live] + 1).float() * 2 * BF16_LOGIT_BAND).all()
    finally:
        decode.release_sessions(m)
