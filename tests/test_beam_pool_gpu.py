"""Beam search with a finished-hypothesis pool on the device: one valor_beam_pool_step launch == decode.beam_pool_step_host bit for bit
(every output array), decode_beam_pool over a scripted session / the re-run source == decode_beam_pool_host, the public interface on
the small synthetic model (reference rule untouched, cached == re-run, graphs on == off, a kept session under both rules, n-best,
sequence_logprobs == forced decoding, an exhaustive answer set, validate_cap), and the early exit."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_beam_pool_cpu as C  # noqa: E402  (the scripts and the independent search of the host-law tests)
import test_constrain_decode_gpu as T  # noqa: E402  (the stub sources and the small synthetic model)

pytestmark = pytest.mark.gpu

EOS = 102
INF = float("inf")
B, V, L, SEP = C.B, C.V, C.L, C.SEP
TERM = 5e-5                                 # per term of a score, as tests/test_answer_set_decode_gpu.py:24 (cached session against re-run)


@pytest.fixture
def sep(monkeypatch):
    from valor_amd import decode
    monkeypatch.setattr(decode, "EOS", SEP)
    return SEP


def same_arrays(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        x, y = (a[k].view(torch.int32), b[k].view(torch.int32)) if a[k].dtype == torch.float32 else (a[k], b[k])
        assert torch.equal(x, y), (k, a[k], b[k])


# ------------------------------------------------------------------------------------------------ one launch == the host law
def random_state(b, K, L_, t, V_, eos, seed, alpha=0.0, dead=(), done=()):
    """a state in the middle of a search: random scores and words, a partly filled pool; dead: (sample, slot) pairs, done: samples"""
    from valor_amd import decode
    g = torch.Generator().manual_seed(seed)
    st = decode.PoolState(b, K, L_, alpha, "cpu", eos)
    i = t % 2
    st.scores[i] = -torch.rand((b, K), generator=g) * 4
    st.scores[1 - i] = torch.full((b, K), 7.0)                                     # what the step must overwrite
    st.hist[i] = torch.randint(3, V_, (b, K, L_), generator=g)
    st.hist[1 - i] = torch.full((b, K, L_), -5)
    for s, k in dead:
        st.scores[i][s, k] = -INF
    for s in range(b):
        n = (s + 1) % (K + 1)                                                       # pools of different fill, one full when b > K - 1
        if s == b - 1:
            n = K
        for j in range(n):
            st.pool_logprob[s, j] = -float(torch.rand((), generator=g)) * 6 - 1
            st.pool_len[s, j] = int(torch.randint(1, max(t, 1) + 1, (), generator=g))
            st.pool_rank[s, j] = st.pool_logprob[s, j] * st.inv[int(st.pool_len[s, j])]
            st.pool_ins[s, j] = (j + s) % n                                             # (distinct, not in slot order)
            st.pool_seq[s, j, :int(st.pool_len[s, j])] = 9
        st.pool_cnt[s, 0], st.pool_cnt[s, 1] = n, n + s
    for s in done:
        st.done[s] = 1
    st.tok.fill_(-1), st.parent.fill_(-1), st.active.fill_(9)
    return st


def launch_equals_law(dev, st, z, t, cur, early=False, beam_major=True, pad=0, lse=None):
    from valor_amd import decode
    zd = z.to(dev)
    if pad:                                                                         # a padded row pitch; the pad holds values that would win
        buf = torch.full((z.shape[0], z.shape[1] + pad), 1e30, device=dev)
        buf[:, :z.shape[1]] = zd
        zd = buf[:, :z.shape[1]]
    lse = decode.row_lse(z.to(dev).contiguous())[0] if lse is None else lse.to(dev)
    host, gpu = st.to("cpu"), st.to(dev)
    decode.beam_pool_step_host(z, lse, host, t, cur, early, beam_major)
    decode.beam_pool_step(zd, lse, gpu, t, cur, early, beam_major)
    torch.cuda.synchronize()
    same_arrays(gpu.arrays(), host.arrays())
    return host


@pytest.mark.parametrize("b,cur,K,V_", [(3, 1, 3, 40), (3, 3, 3, 40), (2, 8, 8, 4099), (1, 1, 1, 2)])
def test_one_launch_equals_the_host_law(dev, b, cur, K, V_):
    from valor_amd import decode
    L_, eos = 6, 1 if V_ == 2 else 2
    g = torch.Generator().manual_seed(b * 100 + cur * 10 + K)
    t = 0 if cur == 1 else 3
    for case in range(4):
        z = torch.randn((b * cur, V_), generator=g)
        z[:, eos] += 1.5                                                            # [SEP] among the leaders: offers, skips and pool replacements
        if case == 1:                                                               # equal logits (index order decides) and -inf columns
            z[0] = 0.25
            z[-1, torch.randperm(V_, generator=g)[:V_ // 2]] = -INF
            z[-1, eos] = 0.0
        alpha = (0.0, 1.0, -1.0, 0.7)[case]
        st = random_state(b, K, L_, t, V_, eos, case, alpha) if t else decode.PoolState(b, K, L_, alpha, "cpu", eos)
        launch_equals_law(dev, st, z, t, cur, early=case == 2, beam_major=case != 3, pad=(0, 5, 0, 29)[case])
    if cur > 1:
        # a sample with dead slots (one of them slot 0), a done sample, both at once; then the last step
        z = torch.randn((b * cur, V_), generator=g)
        st = random_state(b, K, L_, t, V_, eos, 7, 0.0, dead=[(0, 0), (0, K - 1), (b - 1, 1)], done=[b - 1])
        host = launch_equals_law(dev, st, z, t, cur)
        assert host.done[b - 1] == 1 and not host.active[:, b - 1].any()
        st = random_state(b, K, L_, L_ - 1, V_, eos, 8, 1.0, dead=[(0, 1)])
        z[:, eos] += 2.0
        host = launch_equals_law(dev, st, z, L_ - 1, cur)
        assert host.done.all() and not host.active.any()
        # every slot of a sample dead: nothing to take
        st = random_state(b, K, L_, t, V_, eos, 9, 0.0, dead=[(0, k) for k in range(K)])
        host = launch_equals_law(dev, st, z, t, cur)
        assert host.done[0] == 1 and (host.scores[(t + 1) % 2][0] == -INF).all()


def test_all_winners_in_one_threads_stride(dev):
    """V = 4099, K = 8: the 16 winners sit in the columns 5 + 1024 j of the first four rows -- thread 5's stride alone -- with equal values
    among them, and [SEP] is column 5: the walk pools two of them, skips the third (rank 8 = K) and fills its eighth slot at rank 10,
    so a per-thread list shallower than 11 would lose a beam"""
    b, cur, K, V_, L_, eos, t = 2, 8, 8, 4099, 6, 5, 2
    g = torch.Generator().manual_seed(3)
    z = torch.randn((b * cur, V_), generator=g)
    st = random_state(b, K, L_, t, V_, eos, 4)
    st.scores[t % 2][:] = -1.0
    for k in range(4):
        for j in range(4):
            z[k * b:(k + 1) * b, 5 + 1024 * j] = 30.0 - (k * 4 + j) // 2                # pairs of equal values
    host = launch_equals_law(dev, st, z, t, cur, lse=torch.zeros(b * cur))
    assert host.tok.view(K, b)[:, 0].tolist() == [1029, 2053, 3077, 1029, 2053, 3077, 1029, 2053]
    assert host.parent.view(K, b)[:, 0].tolist() == [0, 0, 0, b, b, b, 2 * b, 2 * b]
    # ... and with the floor of an answer set: the floored columns are no continuations, slots stay dead
    z2 = torch.full((b * cur, V_), decode_floor())
    z2[:b, 7], z2[:b, eos], z2[b:2 * b, 4098] = 1.0, 0.5, 0.0
    st = random_state(b, K, L_, t, V_, eos, 5)
    st.floor = decode_floor()
    st.scores[t % 2][:] = -1.0
    host = launch_equals_law(dev, st, z2, t, cur, lse=torch.zeros(b * cur))
    assert host.tok.view(K, b)[:, 0].tolist() == [7, 4098] + [eos] * (K - 2) and host.active[:, 0].tolist() == [1, 1] + [0] * (K - 2)


def decode_floor():
    from valor_amd import decode
    return decode.TRIE_FLOOR


def test_wrapper_refuses_what_the_kernel_cannot_do(dev):
    from valor_amd import decode
    z, l = torch.zeros((3, 40), device=dev), torch.zeros(3, device=dev)
    st = decode.PoolState(3, 3, 8, 0.0, dev, SEP)
    for args in ((z[:, :5].contiguous(), l, st, 0, 1), (z, l, st, 8, 1), (z, l, st, 0, 3), (z.double(), l, st, 0, 1), (z.t().contiguous().t(), l, st, 0, 1)):
        with pytest.raises(ValueError):
            decode.beam_pool_step(*args)
    for kw in (dict(beam=9), dict(beam=0), dict(n_best=4), dict(n_best=0)):
        a = dict(beam=3, n_best=1)
        a.update(kw)
        with pytest.raises(ValueError):
            decode.decode_beam_pool(T.StubSession(C.length_script(), dev), B, a["beam"], L, None, None, a["n_best"])


# ------------------------------------------------------------------------------------------------ the loop over both sources == the host loop
def three_ways(dev, script, b, K, L_, c=None, n=None, early=False):
    from valor_amd import decode
    n = K if n is None else n
    lse = lambda z: decode.row_lse(z.to(dev).contiguous())[0]
    want = decode.decode_beam_pool_host(script, b, K, L_, c, None, n, early, lse=lse)
    sess = T.StubSession(script, dev)
    got = decode.decode_beam_pool(sess, b, K, L_, c, None, n, early)
    rerun = decode.decode_beam_pool(decode._Rerun(T.StubStepper(script, dev, b)), b, K, L_, c, None, n, early)
    for res in (got, rerun):
        same_arrays(dict(zip("srpl", (x.cpu() for x in res))), dict(zip("srpl", want)))
    return want, sess


@pytest.mark.parametrize("K", [1, 3, 8])
def test_loop_over_both_sources_equals_the_host_loop(dev, sep, K):
    from valor_amd import decode
    for alpha, early, seed in ((0.0, False, 0), (1.0, False, 1), (-1.0, True, 2), (0.7, False, 3)):
        script = C.random_script(seed * 10 + K, 3, K, 7, 20, sep)
        three_ways(dev, script, 3, K, 7, decode.Constraints(length_penalty=alpha) if alpha else None, early=early)


def test_length_script_and_constraints_through_the_loops(dev, sep):
    from valor_amd import decode
    script = C.length_script()
    for alpha, want in ((None, [C.H36, C.H30, C.H18]), (1.0, [C.H36, C.H18, C.H09]), (-1.0, [C.H30, C.H36, C.H18])):
        res, _ = three_ways(dev, script, B, 3, L, None if alpha is None else decode.Constraints(length_penalty=alpha))
        assert res[0].tolist() == [want] * B
    ref = decode.decode_beam(T.StubSession(script, dev), B, 3, L).cpu()              # the reference's rule returns the leader and never [10 20 ..]
    assert ref.tolist() == [C.H36] * B
    g = torch.Generator().manual_seed(1)
    script = []
    for t in range(L):                                                               # the script of the reference-rule constraint tests
        z = torch.randn((B * 3, V), generator=g) * 0.5
        z[:, 7] += 4.0 if t % 2 == 0 else 3.0
        z[:, 8] += 3.0 if t % 2 == 0 else 4.0
        z[:, sep] += 2.5 if t >= 4 else -4.0
        script.append(z)
    plain, _ = three_ways(dev, script, B, 3, L)
    assert any(T.repeated_ngrams(r, 2, sep) > 0 for r in plain[0].reshape(-1, L))
    for c in (decode.Constraints(no_repeat_ngram_size=2), decode.Constraints(min_length=6, suppress_tokens=(9, 7)),
              decode.Constraints(repetition_penalty=1.3), decode.Constraints(no_repeat_ngram_size=2, length_penalty=0.7)):
        res, _ = three_ways(dev, script, B, 3, L, c)
        rows = res[0].reshape(-1, L)
        if c.no_repeat_ngram_size or c.min_length:
            assert not torch.equal(res[0], plain[0]), c
        if c.no_repeat_ngram_size:
            assert all(T.repeated_ngrams(r, 2, sep) == 0 for r in rows)
        if c.min_length:
            assert (res[3] >= 6).all() and not (rows == 7).any() and not (rows == 9).any()


def test_early_exit_on_a_scripted_session(dev, sep, monkeypatch):
    from valor_amd import decode
    z = torch.randn((B * 3, V), generator=torch.Generator().manual_seed(2))
    z[:, sep] = 30.0                                                                 # every hypothesis ends at once
    script = [z.clone() for _ in range(L)]
    monkeypatch.setattr(T.StubSession, "poll", 2)
    want, sess = three_ways(dev, script, B, 3, L)
    assert sess.t <= 2                                                               # stepped at most `poll` times
    assert (want[3] <= 2).all() and (want[0][:, 0] == sep).all()
    monkeypatch.setattr(T.StubSession, "poll", 1000)                                 # never asked: all L steps, the same result
    again, sess = three_ways(dev, script, B, 3, L)
    assert sess.t == L
    same_arrays(dict(zip("srpl", again)), dict(zip("srpl", want)))


# ------------------------------------------------------------------------------------------------ the small synthetic model
def forced_logprobs(m, batch, g, seqs, lengths, n):
    """the forced-decoding sum of every returned hypothesis (score_candidates' law: per step valor_xent_fwd's z[label] - lse(z), added in
    fp32 in ascending t) on a session of its own: seqs int64 [b * n, L] clip-major, lengths [b * n] -> fp32 [b * n]"""
    from valor_amd import decode
    with torch.no_grad():
        m.eval()
        b, kv, ranges = decode.encode_for_generation(m, batch, [g])
        rows, Lm = b * n, seqs.shape[1]
        kv_rep = decode._repeat_clips(m, kv, b, n)
        prompt = decode._prompt_rows(m, "caption", rows)
        sess = decode._batch_session(m, rows, 1, kv_rep, prompt, Lm, decode.DecodeSession)
        src = decode._group_source(sess, m, g, rows, kv_rep, ranges, prompt)
        score = torch.zeros(rows, dtype=torch.float32, device=seqs.device)
        for t in range(int(lengths.max())):
            logits = src.step(None if t == 0 else seqs[:, t - 1].contiguous())
            term = decode._forced_terms(logits, seqs[:, t].contiguous())
            score = torch.where(lengths > t, score + term, score)
    return score


def pool_cap(m, batch, groups=("tva", "tv"), **kw):
    return T._cap(m, batch, groups, beam_size=3, beam_search="pool", **kw)


def test_reference_rule_is_untouched_and_a_kept_session_serves_both(dev):
    from valor_amd import decode
    m, spec = T._model(dev)
    batch, qb = T._batch(spec), T._batch(spec, questions=True)
    try:
        plain = T._cap(m, batch, beam_size=3)
        assert set(plain) == {"generated_sequences_t_va", "generated_sequences_t_v"}
        with torch.no_grad():                                                        # ... which is decode_beam's own output
            m.eval()
            b, kv_layers, ranges = decode.encode_for_generation(m, batch, ["tva"])
            direct = decode._decode_groups(m, ["tva"], b, kv_layers, ranges, "caption", 3, 10)["tva"][0].cpu()
        assert torch.equal(direct, plain["generated_sequences_t_va"])
        pool = pool_cap(m, batch)
        T._same(plain, T._cap(m, batch, beam_size=3, beam_search="reference"))       # after a pool search on the same kept session
        T._same(pool, pool_cap(m, batch))
        assert len(m.__dict__["_decode_sessions"]) == 1
        assert set(pool) == {k + g for k in ("generated_sequences_", "sequence_scores_", "sequence_logprobs_") for g in ("t_va", "t_v")}
        qa = T._qa(m, qb, beam_size=3)
        T._same(qa, T._qa(m, qb, beam_size=3, beam_search="reference"))
        qp = T._qa(m, qb, beam_size=3, beam_search="pool", early_stopping=True)
        assert qp["generated_answers_t_va"].shape == (3, 10) and qp["sequence_scores_t_va"].shape == (3,)
        with pytest.raises(ValueError):
            T._cap(m, batch, beam_size=3, num_return_sequences=2)                    # n-best under the reference rule: as before
        for kw in (dict(mode="greedy"), dict(mode="sample"), dict(beam_size=1)):
            with pytest.raises(ValueError, match="pool"):
                T._cap(m, batch, beam_search="pool", **kw)
        for kw in (dict(beam_search="best"), dict(early_stopping=True), dict(beam_search="pool", num_return_sequences=4)):
            with pytest.raises(ValueError):
                T._cap(m, batch, beam_size=3, **kw)
    finally:
        decode.release_sessions(m)


def test_pool_search_cached_rerun_graphs_n_best_and_forced_scores(dev, monkeypatch):
    from valor_amd import decode
    m, spec = T._model(dev)
    batch = T._batch(spec)
    n, Lm = 3, 10
    try:
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "1")
        res = {}
        for name, kw in (("plain", {}), ("ctl", dict(no_repeat_ngram_size=2, length_penalty=0.8, min_length=3)), ("plain_again", {})):
            res[name] = pool_cap(m, batch, num_return_sequences=n, **kw)
        T._same(res["plain"], res["plain_again"])
        for name in ("plain", "ctl"):
            out = res[name]
            for key in ("t_va", "t_v"):
                seqs, sc, lp = out["generated_sequences_" + key], out["sequence_scores_" + key], out["sequence_logprobs_" + key]
                assert seqs.shape == (3 * n, Lm) and sc.shape == lp.shape == (3 * n,)
                assert torch.isfinite(sc).all() and (lp <= 0).all()
                sc3 = sc.view(3, n)
                assert (sc3[:, :-1] >= sc3[:, 1:]).all()                             # sorted by the rank score
                for i in range(3):
                    assert len({tuple(r) for r in seqs[i * n:(i + 1) * n].tolist()}) == n      # distinct
                ended = (seqs == EOS).any(1)
                lengths = torch.where(ended, (seqs == EOS).long().argmax(1) + 1, Lm)
                if name == "ctl":
                    T.check_rows(seqs, 2, 3)
                    assert torch.allclose(sc, lp / lengths.float() ** 0.8, rtol=1e-6, atol=0)
                else:
                    assert torch.equal(sc, lp)
                    g = {"t_va": "tva", "t_v": "tv"}[key]
                    forced = forced_logprobs(m, batch, g, seqs.to(dev), lengths.to(dev), n).cpu()
                    assert ((forced.double() - lp.double()).abs() <= (lengths + 1).double() * TERM).all(), (forced, lp)
        one = pool_cap(m, batch)                                                     # n = 1: the first of the n best
        assert torch.equal(one["generated_sequences_t_va"], res["plain"]["generated_sequences_t_va"][::n])
        monkeypatch.setenv("VALOR_DECODE_GRAPH", "0")
        decode.release_sessions(m)
        for name, kw in (("plain", {}), ("ctl", dict(no_repeat_ngram_size=2, length_penalty=0.8, min_length=3))):
            T._same(res[name], pool_cap(m, batch, num_return_sequences=n, **kw))     # eager steps: bit for bit
        monkeypatch.setenv("VALOR_KV_CACHE", "0")
        decode.release_sessions(m)
        for name, kw in (("plain", {}), ("ctl", dict(no_repeat_ngram_size=2, length_penalty=0.8, min_length=3))):
            rerun = pool_cap(m, batch, num_return_sequences=n, **kw)                 # the re-run path: token for token, scores within the band
            T._same_tokens(res[name], rerun)
            for key in ("t_va", "t_v"):
                assert ((rerun["sequence_logprobs_" + key] - res[name]["sequence_logprobs_" + key]).abs() <= (Lm + 1) * TERM).all()
    finally:
        decode.release_sessions(m)


def test_exhaustive_answer_set_comes_back_whole_in_score_order(dev):
    from valor_amd import decode
    import test_answer_set_decode_gpu as A
    m, spec = T._model(dev)
    _, per = A.model_sets(spec)                                                      # <= 3 answers per sample, pairwise distinct first tokens
    batch = T._batch(spec)
    try:
        out = pool_cap(m, batch, ("tva",), num_return_sequences=3, candidates=per)
        scores = decode.score_candidates(m, batch, ["tva"], per)["tva"].cpu()
        seqs, lp = out["generated_sequences_t_va"].view(3, 3, -1), out["sequence_logprobs_t_va"].view(3, 3)
        for s in range(3):
            c = per.counts[s]
            idx = per.with_roots([s] * c).index_of(seqs[s, :c])
            assert sorted(idx.tolist()) == list(range(c)), (s, idx)                  # the whole set
            got = scores[s, idx]
            assert ((got - lp[s, :c]).abs() <= (per.max_len + 1) * TERM).all()
            assert (got[:-1] >= got[1:] - (per.max_len + 1) * TERM).all()            # in score_candidates' order (within the band of a score)
            assert (seqs[s, c:] == EOS).all() and (lp[s, c:] == -INF).all()          # a set smaller than n: all-[SEP] rows at -inf
    finally:
        decode.release_sessions(m)


def test_model_options_reach_validate_cap_and_the_model_exits_early(dev, tmp_path, monkeypatch):
    from valor_amd import decode
    from valor_amd.evaluate import validate_cap
    m, spec = T._model(dev)
    mo, _ = T._model(dev, generation_beam_search="pool", generation_early_stopping=True, beam_size=3)
    batch = T._batch(spec)
    try:
        mo.beam_size = m.beam_size = 3
        want = pool_cap(m, batch, early_stopping=True)
        T._same(want, T._cap(mo, batch))                                             # the options are the defaults ...
        T._same(T._cap(m, batch), T._cap(mo, batch, beam_search="reference"))        # ... and the call's arguments win
        T._same(T._cap(m, batch, mode="greedy"), T._cap(mo, batch, mode="greedy"))   # no beam search: the option does not apply
        seen = []

        def dec(seqs):
            seen.append(seqs.cpu())
            return [" ".join(f"w{int(x)}" for x in (r[:r.index(EOS)] if EOS in r else r)) or "w0" for r in seqs.tolist()]
        refs = {i: ["w1 w2 w3"] for i in batch["ids"]}
        log = validate_cap(mo, [batch], "cap%tva%tv", refs, decode=dec, scorer="host", output_dir=str(tmp_path), global_step=1)
        assert set(log) == {"tva", "tv"} and len(seen) == 2
        assert torch.equal(seen[0], want["generated_sequences_t_va"]) and torch.equal(seen[1], want["generated_sequences_t_v"])
        # a [SEP] bias far above every word: all hypotheses end in the first two steps, the session is asked once (poll 8) and leaves
        with torch.no_grad():
            m.P["cls.decoder.bias"][EOS] += 40.0
        decode.release_sessions(m)
        early = pool_cap(m, batch, ("tva",), num_return_sequences=3)
        sess = next(iter(m.__dict__["_decode_sessions"].values()))
        assert sess.step_i <= sess.poll < 10
        seqs = early["generated_sequences_t_va"].view(3, 3, -1)
        assert (seqs[:, 0, 0] == EOS).all() and (seqs[:, 1:, 1] == EOS).all()
        monkeypatch.setattr(decode.DecodeSession, "poll", 1000)                      # never asked: all ten steps, the same result
        T._same(early, pool_cap(m, batch, ("tva",), num_return_sequences=3))
        assert next(iter(m.__dict__["_decode_sessions"].values())).step_i == 10
    finally:
        decode.release_sessions(m)
        decode.release_sessions(mo)
