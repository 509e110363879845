"""Diverse (group) beam search on the device: one valor_beam_group_step launch == decode.beam_group_step_host bit for bit (every array
of GroupPoolState, tie-heavy inputs), one group == the valor_beam_pool_step launch, decode_beam_pool with groups over a scripted session
and over the cached session of the small synthetic model == decode_beam_pool_host, and the public interface (generate_cap's shapes,
sequence_groups_*, sequence_logprobs_* == forced decoding, one group == today's call, the model options through validate_cap)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_beam_pool_cpu as C  # noqa: E402  (the random scripts)
import test_beam_pool_gpu as P  # noqa: E402  (same_arrays, random_state, forced_logprobs, TERM)
import test_constrain_decode_gpu as T  # noqa: E402  (the stub sources and the small synthetic model)

pytestmark = pytest.mark.gpu

EOS = 102
INF = float("inf")
SEP = C.SEP
sep = P.sep


# ------------------------------------------------------------------------------------------------ one launch == the host law
def random_group_state(b, K, G, L_, t, V_, eos, seed, alpha=0.0, lam=0.5, dead=(), done=(), gdone=(), quantised=True):
    """a state in the middle of a search: quantised scores (ties across slots), random words, the groups' pool ranges of different
    fill; dead: (sample, slot) pairs, done: samples, gdone: (sample, group) pairs"""
    from valor_amd import decode
    g = torch.Generator().manual_seed(seed)
    Kg = K // G
    st = decode.GroupPoolState(b, K, G, L_, alpha, "cpu", eos, diversity_penalty=lam)
    i = t % 2
    st.scores[i] = -torch.randint(0, 8, (b, K), generator=g).float() * 0.5 if quantised else -torch.rand((b, K), generator=g) * 4
    st.scores[1 - i] = torch.full((b, K), 7.0)                                     # what the step must overwrite
    st.hist[i] = torch.randint(min(3, V_ - 1), V_, (b, K, L_), generator=g)
    st.hist[1 - i] = torch.full((b, K, L_), -5)
    for s, k in dead:
        st.scores[i][s, k] = -INF
    for s in range(b):
        for q in range(G):
            n = Kg if s == b - 1 else (s + q + 1) % (Kg + 1)                        # pool ranges of different fill, the last sample's full
            for j in range(n):
                e = q * Kg + j
                st.pool_logprob[s, e] = -float(torch.rand((), generator=g)) * 6 - 1
                st.pool_len[s, e] = int(torch.randint(1, max(t, 1) + 1, (), generator=g))
                st.pool_rank[s, e] = st.pool_logprob[s, e] * st.inv[int(st.pool_len[s, e])]
                st.pool_ins[s, e] = (j + s) % n                                         # (distinct, not in slot order)
                st.pool_seq[s, e, :int(st.pool_len[s, e])] = 9
            st.pool_cnt[s, q, 0], st.pool_cnt[s, q, 1] = n, n + s
    for s in done:
        st.done[s] = 1
        st.gdone[s] = 1
    for s, q in gdone:
        st.gdone[s, q] = 1
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
    decode.beam_group_step_host(z, lse, host, t, cur, early, beam_major)
    decode.beam_group_step(zd, lse, gpu, t, cur, early, beam_major)
    torch.cuda.synchronize()
    P.same_arrays(gpu.arrays(), host.arrays())
    return host


def quantised_rows(g, rows, V_, eos):
    z = torch.randint(-6, 3, (rows, V_), generator=g).float() * 0.5                 # equal logits inside a row and across rows
    z[:, eos] += 1.5                                                                # [SEP] among the leaders: offers, skips and pool replacements
    return z


@pytest.mark.parametrize("b,cur,K,G,V_", [(3, 1, 4, 2, 40), (3, 4, 4, 2, 40), (2, 8, 8, 4, 4099), (2, 8, 8, 8, 4099), (1, 2, 2, 2, 4)])
def test_one_launch_equals_the_host_law(dev, b, cur, K, G, V_):
    from valor_amd import decode
    L_, eos, Kg = 6, 2, K // G
    g = torch.Generator().manual_seed(b * 1000 + cur * 100 + K * 10 + G)
    t = 0 if cur == 1 else 3
    for case in range(4):
        z = quantised_rows(g, b * cur, V_, eos)
        if case == 1:                                                               # one value everywhere (index order decides) and -inf columns
            z[0] = 0.25
            z[-1, torch.randperm(V_, generator=g)[:V_ // 2]] = -INF
            z[-1, eos] = 0.0
        alpha, lam = (0.0, 1.0, -1.0, 0.7)[case], (0.5, 16.0, 0.0, 1.0)[case]
        st = (random_group_state(b, K, G, L_, t, V_, eos, case, alpha, lam) if t else
              decode.GroupPoolState(b, K, G, L_, alpha, "cpu", eos, diversity_penalty=lam))
        # lse 0 keeps every candidate on the 0.5 grid: a penalised key ties an unpenalised one exactly
        host = launch_equals_law(dev, st, z, t, cur, early=case == 2, beam_major=case != 3, pad=(0, 5, 0, 29)[case],
                                 lse=torch.zeros(b * cur) if case % 2 == 0 else None)
        if case == 0 and V_ > 4:
            toks = host.tok.view(K, b)
            assert any(len(set(toks[:, s].tolist()) - {eos}) > Kg for s in range(b))      # the groups do differ
    if cur > 1:
        # dead slots (a group's first slot, a whole group), a done group, a done sample; then the last step
        z = quantised_rows(g, b * cur, V_, eos)
        dead = [(0, 0), (0, K - 1)] + [(b - 1, k) for k in range(Kg)]
        st = random_group_state(b, K, G, L_, t, V_, eos, 7, 0.0, 0.5, dead=dead, done=[b - 1] if b > 1 else [], gdone=[(0, G - 1)])
        host = launch_equals_law(dev, st, z, t, cur)
        assert host.gdone[0, G - 1] == 1 and not host.active[K - Kg:, 0].any() and host.done[0] == int(K == 2)       # (K = 2: slot 0 was all of group 0)
        if b > 1:
            assert host.done[b - 1] == 1 and not host.active[:, b - 1].any()
        st = random_group_state(b, K, G, L_, L_ - 1, V_, eos, 8, 1.0, 0.5, dead=[(0, 1)], gdone=[(0, 0)])
        z[:, eos] += 2.0
        host = launch_equals_law(dev, st, z, L_ - 1, cur)
        assert host.done.all() and host.gdone.all() and not host.active.any()
        # every slot of a sample dead: nothing to take
        st = random_group_state(b, K, G, L_, t, V_, eos, 9, 0.0, 0.5, dead=[(0, k) for k in range(K)])
        host = launch_equals_law(dev, st, z, t, cur)
        assert host.done[0] == 1 and (host.scores[(t + 1) % 2][0] == -INF).all()
        # the floor of an answer set: floored columns are no continuations, slots stay dead
        z2 = torch.full((b * cur, V_), decode.TRIE_FLOOR)
        z2[:, eos] = 0.5
        z2[:b, 3], z2[:b, 1] = 1.0, 0.0                                              # (the rows of slot 0: the only words left)
        st = random_group_state(b, K, G, L_, t, V_, eos, 10, 0.0, 16.0)
        st.floor = decode.TRIE_FLOOR
        host = launch_equals_law(dev, st, z2, t, cur, lse=torch.zeros(b * cur))
        assert set(host.tok.tolist()) <= {1, 3, eos} and (host.active.sum(0) < K).all()


def test_all_of_a_groups_winners_in_one_threads_stride(dev):
    """V = 4099, K = 8. Two groups (Kg = 4, lists of depth 8): the 8 winners of either group sit in the columns 5 + 1024 j of the group's
    first two rows -- thread 5's stride alone -- in pairs of equal values, [SEP] is column 5, and group 1 pays for the words group 0
    took. One group (Kg = 8, depth 16): the pool kernel's case, 16 winners in that stride."""
    b, cur, K, V_, L_, eos, t = 2, 8, 8, 4099, 6, 5, 2
    g = torch.Generator().manual_seed(3)
    for G, lam in ((2, 0.5), (2, 64.0), (1, 0.0)):
        Kg = K // G
        z = torch.randn((b * cur, V_), generator=g)
        st = random_group_state(b, K, G, L_, t, V_, eos, 4, lam=lam)
        st.scores[t % 2][:] = -1.0
        for q in range(G):
            for kk in range(Kg // 2):
                k = q * Kg + kk
                for j in range(4):
                    z[k * b:(k + 1) * b, 5 + 1024 * j] = 30.0 - (kk * 4 + j) // 2            # pairs of equal values
        host = launch_equals_law(dev, st, z, t, cur, lse=torch.zeros(b * cur))
        toks = host.tok.view(K, b)[:, 0].tolist()
        if G == 1:                                                                   # tests/test_beam_pool_gpu.py's figures
            assert toks == [1029, 2053, 3077, 1029, 2053, 3077, 1029, 2053]
        else:
            assert toks[:Kg] == [1029, 2053, 3077, 1029]
            assert set(toks[Kg:]) <= {1029, 2053, 3077} if lam < 1 else not set(toks[Kg:]) & {1029, 2053, 3077}


def test_a_penalised_word_that_is_the_best_candidate_of_several_slots(dev):
    """K = 4, G = 2: word 7 is the best continuation of all four slots. Group 0 takes it from both its slots; both slots of group 1 see it
    at c - pen[2], and what group 1 takes instead depends on the penalty: 7 twice (0.25), one 7 and one 9 (1.5: an exact tie), 9 twice (4)"""
    b, K, G, V_, L_, eos, t = 2, 4, 2, 40, 6, 2, 2
    for lam, want in ((0.25, [7, 7, 7, 7]), (1.5, [7, 7, 7, 9]), (4.0, [7, 7, 9, 9])):
        z = torch.full((b * K, V_), -9.0)
        z[:, 7], z[:, 9], z[:, 11] = 0.0, -3.0, -8.5
        st = random_group_state(b, K, G, L_, t, V_, eos, 2, lam=lam)
        st.scores[t % 2][:] = torch.tensor([-1.0, -1.5, -1.0, -1.0])
        st.pool_cnt.zero_()
        host = launch_equals_law(dev, st, z, t, K, lse=torch.zeros(b * K))
        # group 1: word 7 at -1 - 2 * penalty in both slots, word 9 at -4 in both. 0.25: -1.5, both 7s. 1.5: four keys of -4, in
        # index order (slot 2: 7), (slot 2: 9), (slot 3: 7), (slot 3: 9) -- the first two, both of slot 2. 4: -9, the two 9s.
        assert host.tok.view(K, b)[:, 0].tolist() == want, lam
        assert host.scores[(t + 1) % 2][0].tolist() == [-1.0, -1.5] + [-1.0 if w == 7 else -4.0 for w in want[2:]]      # unpenalised
        assert host.parent.view(K, b)[2:, 0].tolist() == ([2 * b, 2 * b] if lam == 1.5 else [2 * b, 3 * b])


def test_one_group_launch_equals_the_pool_launch(dev):
    from valor_amd import decode
    for b, cur, K, V_ in ((3, 3, 3, 40), (2, 8, 8, 4099), (3, 1, 4, 40)):
        L_, eos = 6, 2
        t = 0 if cur == 1 else 3
        g = torch.Generator().manual_seed(K)
        z = quantised_rows(g, b * cur, V_, eos)
        pool = P.random_state(b, K, L_, t, V_, eos, 1, 0.7, dead=[(0, 1)] if cur > 1 else ()) if t else decode.PoolState(b, K, L_, 0.7, "cpu", eos)
        grp = decode.GroupPoolState(b, K, 1, L_, 0.7, "cpu", eos)
        for name in decode.PoolState.FIELDS:
            v = getattr(pool, name)
            setattr(grp, name, [x.clone() for x in v] if isinstance(v, list) else v.clone().reshape(getattr(grp, name).shape))
        grp.gdone = pool.done.clone().reshape(b, 1)
        pd, gd = pool.to(dev), grp.to(dev)
        lse = decode.row_lse(z.to(dev))[0]
        decode.beam_pool_step(z.to(dev), lse, pd, t, cur)
        decode.beam_group_step(z.to(dev), lse, gd, t, cur)
        torch.cuda.synchronize()
        pa, ga = pd.arrays(), gd.arrays()
        P.same_arrays(pa, {k: ga[k].reshape(pa[k].shape) for k in pa})
        assert torch.equal(ga["gdone"].reshape(-1), ga["done"])


def test_wrapper_refuses_what_the_kernel_cannot_do(dev):
    from valor_amd import decode, lib
    z, l = torch.zeros((4, 40), device=dev), torch.zeros(4, device=dev)
    st = decode.GroupPoolState(1, 4, 2, 8, 0.0, dev, SEP, diversity_penalty=1.0)
    for args in ((z[:1, :3].contiguous(), l[:1], st, 0, 1), (z[:2], l[:2], st, 1, 2), (z[:3], l[:3], st, 1, 3), (z, l, st, 8, 4),
                 (z.double(), l, st, 1, 4), (z.t().contiguous().t(), l, st, 1, 4), (z[:1], l, st, 0, 1)):
        with pytest.raises(ValueError):
            decode.beam_group_step(*args)
    for kw in (dict(num_beam_groups=3), dict(num_beam_groups=2, diversity_penalty=-1.0), dict(num_beam_groups=2, diversity_penalty=INF),
               dict(num_beam_groups=1, diversity_penalty=1.0), dict(num_beam_groups=2, n_best=5)):
        sess = T.StubSession(C.random_script(0, 3, 4, 7, 20, SEP), dev)
        with pytest.raises(ValueError):
            decode.decode_beam_pool(sess, 3, 4, 7, None, None, kw.pop("n_best", 1), **kw)
        assert sess.t == 0                                                           # before any step
    # the entry point's own refusals, before any launch
    ok = [0, z.data_ptr(), 40, 1, 1, l.data_ptr(), st.scores[0].data_ptr(), st.hist[0].data_ptr(), st.inv.data_ptr(), st.pen.data_ptr(), 1, 1, 40,
          4, 2, 8, 0, SEP, -INF, 0, 0, st.scores[1].data_ptr(), st.hist[1].data_ptr(), st.tok.data_ptr(), st.parent.data_ptr(),
          st.active.data_ptr(), st.pool_seq.data_ptr(), st.pool_logprob.data_ptr(), st.pool_rank.data_ptr(), st.pool_len.data_ptr(),
          st.pool_ins.data_ptr(), st.pool_cnt.data_ptr(), st.gdone.data_ptr(), st.done.data_ptr()]
    before = st.arrays()
    for pos, bad in ((14, 3), (14, 0), (14, 5), (11, 2), (12, 3), (9, 0), (32, 0), (13, 9), (16, 8)):
        args = list(ok)
        args[pos] = bad
        with pytest.raises(lib.ValorHipError):
            lib.call("valor_beam_group_step", *args)
    torch.cuda.synchronize()
    P.same_arrays(st.arrays(), before)


# ------------------------------------------------------------------------------------------------ the loop == the host loop
def loops_agree(dev, script, b, K, G, L_, lam, c=None, a=None, early=False):
    from valor_amd import decode
    lse = lambda z: decode.row_lse(z.to(dev).contiguous())[0]
    want = decode.decode_beam_pool_host(script, b, K, L_, c, a, K, early, lse=lse, num_beam_groups=G, diversity_penalty=lam)
    sess = T.StubSession(script, dev)
    got = decode.decode_beam_pool(sess, b, K, L_, c, a, K, early, G, lam)
    P.same_arrays(dict(zip("srplg", (x.cpu() for x in got))), dict(zip("srplg", want)))
    return want


@pytest.mark.parametrize("K,G", [(4, 2), (8, 4)])
def test_loop_over_a_scripted_session_equals_the_host_loop(dev, sep, K, G):
    from valor_amd import decode
    b, L_, V_ = 3, 7, 24
    for lam, c, early, seed in ((0.5, None, False, 0), (16.0, decode.Constraints(length_penalty=1.0), False, 1),
                                (1.0, decode.Constraints(length_penalty=-1.0), True, 2),
                                (0.5, decode.Constraints(no_repeat_ngram_size=2, length_penalty=0.7), False, 3)):
        script = C.random_script(seed * 10 + K, b, K, L_, V_, sep)
        res = loops_agree(dev, script, b, K, G, L_, lam, c, None, early)
        assert res[4][:, :G].sort(1)[0].tolist() == [list(range(G))] * b              # the first G: one hypothesis per group
        if c is not None and c.no_repeat_ngram_size:
            assert all(T.repeated_ngrams(r, 2, sep) == 0 for r in res[0].reshape(-1, L_))
    # inside an answer set: every returned row is a candidate (or missing), and the groups spread over the set
    aset = decode.AnswerSet([[7, 8, 9], [7, 8], [7, 5], [20], [10, 11, 12, 13], [10, 3], [4], [6, 6]]).for_rows(b)
    script = C.random_script(77 + K, b, K, L_, V_, sep)
    seqs, rank, logp, length, group = loops_agree(dev, script, b, K, G, L_, 4.0, decode.Constraints(length_penalty=0.7), aset)
    found = rank > -INF
    assert found[:, :G].all() and (aset.index_of(seqs.reshape(-1, L_)[found.reshape(-1)]) >= 0).all()


# ------------------------------------------------------------------------------------------------ the small synthetic model
def group_cap(m, batch, groups=("tva", "tv"), **kw):
    return T._cap(m, batch, groups, beam_size=4, beam_search="pool", **kw)


def test_loop_over_the_cached_session_equals_the_host_loop(dev):
    from valor_amd import decode
    import test_answer_set_decode_gpu as A
    m, spec = T._model(dev)
    batch = T._batch(spec)
    shared, _ = A.model_sets(spec)
    Lm = 10
    lse = lambda z: decode.row_lse(z.to(dev).contiguous())[0]                        # (under a logits rule the host loop's rows are host rows)
    try:
        with torch.no_grad():
            m.eval()
            b, kv, ranges = decode.encode_for_generation(m, batch, ["tva"])
            prompt = decode._prompt_rows(m, "caption", b)
            for K, G, lam, c, a in ((4, 2, 1.0, decode.Constraints(no_repeat_ngram_size=2, length_penalty=0.8), None),
                                    (8, 4, 0.5, decode.Constraints(length_penalty=0.8), None),
                                    (4, 2, 2.0, None, shared.for_rows(b))):
                sess = decode._batch_session(m, b, K, kv, prompt, Lm, decode.DecodeSession)
                got = decode.decode_beam_pool(decode._group_source(sess, m, "tva", b, kv, ranges, prompt), b, K, Lm, c, a, K, False, G, lam)
                got = [x.cpu() for x in got]
                want = decode.decode_beam_pool_host(decode._group_source(sess, m, "tva", b, kv, ranges, prompt), b, K, Lm, c, a, K, False,
                                                    lse=lse, num_beam_groups=G, diversity_penalty=lam)
                P.same_arrays(dict(zip("srplg", got)), dict(zip("srplg", want)))
                del sess
    finally:
        decode.release_sessions(m)


def test_generate_cap_with_groups_forced_scores_one_group_and_the_model_options(dev, tmp_path):
    from valor_amd import decode
    from valor_amd.evaluate import validate_cap
    m, spec = T._model(dev)
    mo, _ = T._model(dev, generation_beam_search="pool", generation_num_beam_groups=2, generation_diversity_penalty=1.5, beam_size=4)
    batch = T._batch(spec)
    n, Lm, G = 4, 10, 2
    try:
        mo.beam_size = m.beam_size = 4
        today = group_cap(m, batch, num_return_sequences=n)
        T._same(today, group_cap(m, batch, num_return_sequences=n, num_beam_groups=1, diversity_penalty=0.0))       # one group: today's call
        assert not any(k.startswith("sequence_groups_") for k in today)
        out = group_cap(m, batch, num_return_sequences=n, num_beam_groups=G, diversity_penalty=1.5)
        assert set(out) == {k + g for k in ("generated_sequences_", "sequence_scores_", "sequence_logprobs_", "sequence_groups_") for g in ("t_va", "t_v")}
        for key in ("t_va", "t_v"):
            seqs, sc, lp, gr = (out[k + key] for k in ("generated_sequences_", "sequence_scores_", "sequence_logprobs_", "sequence_groups_"))
            assert seqs.shape == (3 * n, Lm) and sc.shape == lp.shape == gr.shape == (3 * n,) and gr.dtype == torch.int64
            assert torch.isfinite(sc).all() and (lp <= 0).all() and torch.equal(sc, lp)                               # length_penalty 0
            assert gr.view(3, n)[:, :G].sort(1)[0].tolist() == [[0, 1]] * 3 and sorted(gr.view(3, n)[0].tolist()) == [0, 0, 1, 1]
            sc3, gr3 = sc.view(3, n), gr.view(3, n)
            assert (sc3[:, 0] >= sc3[:, 1]).all() and (sc3[:, 2] >= sc3[:, 3]).all()                                  # by score within a place
            for i in range(3):
                for q in range(G):
                    mine = sc3[i][gr3[i] == q]
                    assert (mine[:-1] >= mine[1:]).all()                                                              # by place within a group
            ended = (seqs == EOS).any(1)
            lengths = torch.where(ended, (seqs == EOS).long().argmax(1) + 1, Lm)
            forced = P.forced_logprobs(m, batch, {"t_va": "tva", "t_v": "tv"}[key], seqs.to(dev), lengths.to(dev), n).cpu()
            assert ((forced.double() - lp.double()).abs() <= (lengths + 1).double() * P.TERM).all(), (forced, lp)     # true log-probabilities
        assert torch.equal(group_cap(m, batch, num_beam_groups=G, diversity_penalty=1.5)["generated_sequences_t_va"],
                           out["generated_sequences_t_va"][::n])                                                       # n = 1: the overall best
        for kw in (dict(num_beam_groups=3), dict(num_beam_groups=2, diversity_penalty=-1.0), dict(diversity_penalty=1.0),
                   dict(num_beam_groups=2, num_return_sequences=5), dict(num_beam_groups=2, diversity_penalty=float("nan"))):
            with pytest.raises(ValueError):
                group_cap(m, batch, **kw)
        with pytest.raises(ValueError, match="pool"):
            T._cap(m, batch, beam_size=4, num_beam_groups=2)
        qb = T._batch(spec, questions=True)
        qa = T._qa(m, qb, beam_size=4, beam_search="pool", num_beam_groups=2, diversity_penalty=1.5)
        assert qa["generated_answers_t_va"].shape == (3, Lm) and qa["sequence_groups_t_va"].shape == (3,)
        # the model options alone: the same result, and validate_cap reaches them
        want = group_cap(m, batch, num_beam_groups=G, diversity_penalty=1.5)
        T._same(want, T._cap(mo, batch))
        T._same(T._cap(m, batch, beam_size=4), T._cap(mo, batch, beam_search="reference", num_beam_groups=1, diversity_penalty=0.0))
        with pytest.raises(ValueError, match="options"):                             # groups from the options under the reference rule
            T._cap(mo, batch, beam_search="reference")
        T._same(T._cap(m, batch, mode="greedy"), T._cap(mo, batch, mode="greedy"))   # no beam search: the options do not apply
        seen = []

        def dec(seqs):
            seen.append(seqs.cpu())
            return [" ".join(f"w{int(x)}" for x in (r[:r.index(EOS)] if EOS in r else r)) or "w0" for r in seqs.tolist()]
        refs = {i: ["w1 w2 w3"] for i in batch["ids"]}
        log = validate_cap(mo, [batch], "cap%tva%tv", refs, decode=dec, scorer="host", output_dir=str(tmp_path), global_step=1)
        assert set(log) == {"tva", "tv"} and len(seen) == 2
        assert torch.equal(seen[0], want["generated_sequences_t_va"]) and torch.equal(seen[1], want["generated_sequences_t_v"])
    finally:
        decode.release_sessions(m)
        decode.release_sessions(mo)
