"""The law of the beam search with a finished-hypothesis pool, on the host (no GPU): decode.decode_beam_pool_host against an independent
plain-Python search (lists, numpy fp32 scalars, a sorted pool), the hand-derived n-best of the `length_script` geometry (which the
reference-rule search cannot produce), the edge rules of one step (beam_pool_step_host) and the argument checks."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import decode  # noqa: E402

INF = float("inf")
B, V, L, SEP = 3, 40, 8, 2                  # the scripted geometry of tests/test_constrain_decode_gpu.py; its [SEP] is column 2
f32 = np.float32


def bits(x):
    return x.contiguous().view(torch.int32)


def lse_rows(z):
    return torch.logsumexp(z.to(torch.float32), 1)


# ------------------------------------------------------------------------------------------------ an independent search, for clarity
def plain_pool_search(script, b, K, L_, alpha, early, eos, n):
    """Beam search with a finished-hypothesis pool, one sample at a time, on Python lists. script[t]: logits [>= K * b, V_], rows
    beam-major. -> per sample the n best as (words padded with eos, length, rank, logP)."""
    V_ = script[0].shape[1]
    inv = [f32(1.0)] + [f32(1.0 / float(l) ** alpha) for l in range(1, L_ + 1)]
    lses = [lse_rows(z).numpy() for z in script]
    rows = [z.numpy() for z in script]
    out = []
    for s in range(b):
        beams = [(f32(0.0), [])]                                     # the open hypotheses, best first: (logP, words); the list index is the slot
        pool, inserted = [], 0                                       # finished: dicts
        for t in range(L_):
            cands = []
            for k, (ck, _) in enumerate(beams):
                r = k * b + s
                for w in range(V_):
                    c = f32(ck + f32(rows[t][r, w] - lses[t][r]))
                    if c > -INF:
                        cands.append((c, k * V_ + w))
            cands.sort(key=lambda cw: (-float(cw[0]), cw[1]))
            new, counted = [], 0
            for rho, (c, ix) in enumerate(cands[:2 * K]):
                if counted == K:
                    break
                k, w = divmod(ix, V_)
                words = beams[k][1] + [w]
                if w == eos:
                    if rho >= K:
                        continue
                    offer = (words, t + 1)
                else:
                    counted += 1
                    new.append((c, words))
                    if t < L_ - 1:
                        continue
                    offer = (words, L_)
                rank = f32(c * inv[offer[1]])
                entry = dict(words=offer[0], length=offer[1], rank=rank, logp=c, ins=inserted)
                if len(pool) < K:
                    pool.append(entry)
                    inserted += 1
                else:
                    worst = min(pool, key=lambda e: (float(e["rank"]), -e["ins"]))
                    if rank > worst["rank"]:
                        pool[pool.index(worst)] = entry
                        inserted += 1
            beams = new
            if t == L_ - 1 or not beams:
                break
            if len(pool) == K:
                worst = min(float(e["rank"]) for e in pool)
                if early or worst >= float(f32(beams[0][0] * inv[L_ if alpha > 0 else t + 2])):
                    break
        best = sorted(pool, key=lambda e: (-float(e["rank"]), e["ins"]))[:n]
        out.append([(e["words"] + [eos] * (L_ - len(e["words"])), e["length"], e["rank"], e["logp"]) for e in best])
    return out


def random_script(seed, b, K, L_, V_, eos):
    """quantised logits (ties inside a row), every slot of a sample reading the SAME row at odd steps (ties across slots), [SEP] strong
    from the middle on (hypotheses end at different steps)"""
    g = torch.Generator().manual_seed(seed)
    script = []
    for t in range(L_):
        z = torch.randint(-6, 3, (K * b, V_), generator=g).float() * 0.5
        if t % 2 == 1:
            z = z[:b].repeat(K, 1)
        z[:, eos] = torch.randint(-4, 5, (K * b,), generator=g).float() * 0.5 + (1.0 if t >= L_ // 2 else -1.0)
        script.append(z)
    return script


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("alpha", [0.0, 1.0, -1.0, 0.7])
@pytest.mark.parametrize("early", [False, True])
def test_host_law_equals_an_independent_search(K, alpha, early):
    b, L_, V_, eos = 3, 7, 20, 2
    c = decode.Constraints(length_penalty=alpha) if alpha else None
    for seed in (0, 1, 2):
        script = random_script(seed * 10 + K, b, K, L_, V_, eos)
        assert all(len(set(row.tolist())) < V_ for z in script for row in z)                    # every row holds equal logits: index order decides
        seqs, rank, logp, length = decode.decode_beam_pool_host(script, b, K, L_, c, None, K, early, eos=eos)
        want = plain_pool_search(script, b, K, L_, alpha, early, eos, K)
        assert seqs.shape == (b, K, L_) and rank.shape == logp.shape == length.shape == (b, K)
        for s in range(b):
            n = len(want[s])
            assert n >= 1
            for j, (words, ln, rk, lp) in enumerate(want[s]):
                assert seqs[s, j].tolist() == words and int(length[s, j]) == ln, (seed, s, j)
                assert bits(rank[s, j:j + 1]).item() == np.array([rk], dtype=f32).view(np.int32)[0], (seed, s, j)
                assert bits(logp[s, j:j + 1]).item() == np.array([lp], dtype=f32).view(np.int32)[0], (seed, s, j)
            assert (seqs[s, n:] == eos).all() and (rank[s, n:] == -INF).all() and (length[s, n:] == 0).all()


# ------------------------------------------------------------------------------------------------ the length_script geometry
def length_script():
    """tests/test_constrain_decode_gpu.py::length_script, copied: beam 3, the same for every sample. Step 0: 10 (p .5), 11 (.4), 12 (.1).
    Step 1: after 10, [SEP] (.6) or 20 (.4); after 11, 21; after 12, 22. Then 22 23 24 25 26 with p 1, and at the last step [SEP]
    (.9) or 39 (.1)."""
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


H36 = [11, 21, 22, 23, 24, 25, 26, SEP]      # p .4 * .9
H30 = [10, SEP] + [SEP] * 6                  # p .5 * .6
H18 = [10, 20, 22, 23, 24, 25, 26, SEP]      # p .5 * .4 * .9
H09 = [12, 22, 22, 23, 24, 25, 26, SEP]      # p .1 * .9


def reference_rule_beams(script, s, beam, eos):
    """the reference's rule on lists (decode_beam's law): an ended beam stays and its score stands for every word -> the final beams"""
    V_ = script[0].shape[1]
    beams = [(0.0, [], False)]
    for t in range(len(script)):
        cands = []
        for k, (ck, words, ended) in enumerate(beams):
            lp = torch.log_softmax(script[t][k * B + s].double(), 0).tolist()
            for w in range(V_):
                cands.append((ck if ended else ck + lp[w], k * V_ + w))
        cands.sort(key=lambda cw: (-cw[0], cw[1]))
        beams = [(c, beams[ix // V_][1] + [ix % V_], beams[ix // V_][2] or ix % V_ == eos) for c, ix in cands[:beam]]
    return beams


def test_length_script_n_best():
    """By hand (K = 3, L = 8; p = the product of the step probabilities, the -40 columns carry no mass):
    step 0 opens [10] .5, [11] .4, [12] .1. Step 1: candidates [11 21] .4, [10 SEP] .3, [10 20] .2, [12 22] .1 -> [10 SEP] is pooled at
    rank 1 (length 2), the three others stay open. Steps 2-6 extend them with p 1. The last step offers the three ... [SEP] endings at
    ranks 0-2 (p .36, .18, .09; length 8), then the ... 39 endings (.04, .02, .01). The pool holds 3:
      alpha  0: rank = ln p.       .36 and .18 fill the pool beside .3; .09 < .18 loses.       n-best: .36, .3, .18
      alpha  1: rank = ln p / len. ln .36 / 8 = -.128, ln .18 / 8 = -.214, ln .3 / 2 = -.602; the full pool's worst is [10 SEP] and
                ln .09 / 8 = -.301 beats it; ln .04 / 8 = -.402 does not beat -.301.            n-best: .36, .18, .09
      alpha -1: rank = ln p * len. ln .3 * 2 = -2.41, ln .36 * 8 = -8.17, ln .18 * 8 = -13.7; .09 (-19.3) loses.  n-best: .3, .36, .18
    (length normalisation with alpha = 1 favours the three long endings over [10 SEP]: the ranking acts INSIDE the search.)"""
    script = length_script()
    for alpha, want in ((None, [H36, H30, H18]), (0.0, [H36, H30, H18]), (1.0, [H36, H18, H09]), (-1.0, [H30, H36, H18])):
        c = None if alpha is None else decode.Constraints(length_penalty=alpha)
        seqs, rank, logp, length = decode.decode_beam_pool_host(script, B, 3, L, c, None, 3, False, eos=SEP)
        assert seqs.tolist() == [want] * B, (alpha, seqs[0])
        assert length[0].tolist() == [2 if h is H30 else 8 for h in want]
        assert (rank[:, :-1] >= rank[:, 1:]).all()
        p = {id(H36): .36, id(H30): .3, id(H18): .18, id(H09): .09}
        assert torch.allclose(logp[0], torch.tensor([math.log(p[id(h)]) for h in want]), atol=1e-5)
        a = alpha or 0.0
        assert torch.allclose(rank[0], torch.tensor([math.log(p[id(h)]) / (2 if h is H30 else 8) ** a for h in want]), atol=1e-5)
    # the condition of the test: the reference's rule cannot return the third hypothesis -- copies of [10 SEP] take its place
    final = [words for _, words, _ in reference_rule_beams(script, 0, 3, SEP)]
    assert final[0] == H36 and all(words[:2] == [10, SEP] for words in final[1:])
    assert all(words[:len(H18)] != H18 for words in final)
    # the pool's state after step 1: [10 SEP] pooled, [11 21], [10 20], [12 22] open
    st = decode.PoolState(B, 3, L, 0.0, "cpu", SEP)
    for t in range(2):
        z = script[t][:B * (1 if t == 0 else 3)]
        decode.beam_pool_step_host(z, lse_rows(z), st, t, 1 if t == 0 else 3)
    assert st.pool_cnt.tolist() == [[1, 1]] * B and st.pool_seq[0, 0, :2].tolist() == [10, SEP] and st.pool_len[:, 0].tolist() == [2] * B
    assert st.hist[0][0, :, :2].tolist() == [[11, 21], [10, 20], [12, 22]] and st.parent.tolist() == [3, 4, 5, 0, 1, 2, 6, 7, 8]
    assert st.active.all() and not st.done.any()


# ------------------------------------------------------------------------------------------------ the edge rules of one step
def one_hot_rows(rows, V_, entries, lo=-INF):
    z = torch.full((rows, V_), lo)
    for r, w, v in entries:
        z[r, w] = v
    return z


def step(st, z, t, cur, **kw):
    return decode.beam_pool_step_host(z, torch.zeros(z.shape[0]), st, t, cur, **kw)      # lse 0: the logits are the log-probabilities


def test_sep_at_rank_k_minus_1_is_pooled_and_at_rank_k_skipped():
    K, V_, L_ = 2, 8, 4
    st = decode.PoolState(1, K, L_, 0.0, "cpu", SEP)
    step(st, one_hot_rows(1, V_, [(0, 5, -1.0), (0, SEP, -2.0), (0, 6, -3.0), (0, 7, -4.0)]), 0, 1)
    assert st.pool_cnt.tolist() == [[1, 1]] and st.pool_seq[0, 0].tolist() == [SEP] * L_ and st.pool_len[0, 0] == 1      # rank 1 = K - 1
    assert st.tok.tolist() == [5, 6] and st.scores[1].tolist() == [[-1.0, -3.0]]
    # two rows: [SEP] of slot 0 at rank 0 (pooled), 5 at rank 1, [SEP] of slot 1 at rank 2 = K (skipped), 6 at rank 3
    z = one_hot_rows(2, V_, [(0, SEP, -0.5), (0, 5, -1.0), (1, SEP, -0.5), (1, 6, -2.0)])
    step(st, z, 1, 2)
    assert st.pool_cnt.tolist() == [[2, 2]] and st.pool_seq[0, 1].tolist() == [5, SEP, SEP, SEP] and st.pool_len[0].tolist() == [1, 2]
    assert st.tok.tolist() == [5, 6] and st.parent.tolist() == [0, 1]
    assert st.scores[0].tolist() == [[-2.0, -5.0]] and st.hist[0][0].tolist() == [[5, 5, 0, 0], [6, 6, 0, 0]]


def test_minus_inf_is_never_taken_and_dead_slots_terminate():
    K, V_, L_ = 3, 8, 5
    st = decode.PoolState(2, K, L_, 0.0, "cpu", SEP)
    z = one_hot_rows(2, V_, [(0, 4, -1.0), (1, 4, -1.0), (1, 5, -1.5), (1, 6, -2.0), (1, 7, -2.5)])
    step(st, z, 0, 1)
    assert st.scores[1].tolist() == [[-1.0, -INF, -INF], [-1.0, -1.5, -2.0]]                 # sample 0: one continuation, two dead slots
    assert st.tok.view(K, 2).t().tolist() == [[4, SEP, SEP], [4, 5, 6]]
    assert st.parent.view(K, 2).t().tolist() == [[0, 2, 4], [1, 1, 1]]                       # a dead slot continues itself
    assert st.active.t().tolist() == [[1, 0, 0], [1, 1, 1]] and not st.done.any()
    # a dead slot supplies no candidates even where its row is finite; a sample without a live continuation is done
    z = torch.zeros((K * 2, V_))
    z[0] = -INF                                                                              # slot 0 of sample 0: nothing allowed
    step(st, z, 1, K)
    assert st.done.tolist() == [1, 0] and not st.active[:, 0].any() and st.scores[0][0].tolist() == [-INF] * 3
    # the loop over a script whose rows allow a single chain ends with that chain alone
    script = [one_hot_rows(K, V_, [(k, 3 + t, -0.5) for k in range(K)] + ([(k, SEP, -0.25) for k in range(K)] if t == 3 else []))
              for t in range(L_)]
    seqs, rank, logp, length = decode.decode_beam_pool_host(script, 1, K, L_, None, None, K, eos=SEP)
    assert seqs[0].tolist() == [[3, 4, 5, SEP, SEP], [3, 4, 5, 6, 7], [SEP] * 5] and length.tolist() == [[4, 5, 0]]
    lse3 = math.log(math.exp(-0.5) + math.exp(-0.25))                                        # the only step with a choice
    assert torch.allclose(logp[0, :2], torch.tensor([-0.25 - lse3, -0.5 - lse3]), atol=1e-6) and logp[0, 2] == -INF


def full_pool(ranks, K, L_):
    st = decode.PoolState(1, K, L_, 0.0, "cpu", SEP)
    for j, r in enumerate(ranks):
        st.pool_rank[0, j] = st.pool_logprob[0, j] = r
        st.pool_ins[0, j], st.pool_len[0, j] = j, 1
        st.pool_seq[0, j, 0] = 20 + j
    st.pool_cnt[0, 0] = st.pool_cnt[0, 1] = len(ranks)
    return st


def test_pool_ties_keep_the_older_entry():
    K, V_, L_ = 2, 8, 6
    st = full_pool([-1.0, -1.0], K, L_)
    step(st, one_hot_rows(1, V_, [(0, SEP, -1.0), (0, 5, -1.5), (0, 6, -1.75)]), 0, 1)       # an equal offer does not enter
    assert st.pool_ins.tolist() == [[0, 1]] and st.pool_cnt.tolist() == [[2, 2]]
    assert st.done.tolist() == [1]                                                           # -1 >= -1.5: nothing open can still enter
    st = full_pool([-1.0, -1.0], K, L_)
    step(st, one_hot_rows(1, V_, [(0, SEP, -0.5), (0, 5, -0.75), (0, 6, -0.8)]), 0, 1)       # a better one replaces the NEWER of the two
    assert st.pool_ins.tolist() == [[0, 2]] and st.pool_rank.tolist() == [[-1.0, -0.5]] and st.pool_seq[0, 1].tolist() == [SEP] * L_
    assert st.done.tolist() == [0]                                                           # -1 < -0.75: the open beam may still enter
    seqs, rank, _, _ = st.result(2)
    assert rank.tolist() == [[-0.5, -1.0]] and seqs[0, 1, 0] == 20
    st = full_pool([-1.0, -1.0], K, L_)                                                      # equal ranks come out oldest first
    assert st.result(2)[0][0, :, 0].tolist() == [20, 21]


def test_done_sample_is_frozen_and_early_stopping():
    K, V_, L_ = 2, 8, 6
    for early in (False, True):
        st = decode.PoolState(2, K, L_, 0.0, "cpu", SEP)
        z = one_hot_rows(2, V_, [(0, SEP, -0.1), (0, 5, -3.0), (0, 6, -4.0), (1, 5, -1.0), (1, 6, -2.0), (1, 7, -3.0)])
        step(st, z, 0, 1, early_stopping=early)
        assert st.pool_cnt[:, 0].tolist() == [1, 0] and not st.done.any()
        z = one_hot_rows(4, V_, [(0, SEP, -0.1), (0, 5, -9.0), (2, 5, -9.0), (2, 6, -9.5), (1, 5, -1.0), (3, 5, -1.0), (1, 6, -2.0), (3, 6, -2.0)])
        step(st, z, 1, K, early_stopping=early)
        # sample 0: the pool holds [SEP] (-0.1) and [5 SEP] (-3.1); the best open beam has -12: done under either rule here
        assert st.pool_cnt[:, 0].tolist() == [2, 0] and st.done.tolist() == [1, 0]
        before = {k: v.clone() for k, v in st.arrays().items()}
        step(st, torch.zeros((4, V_)), 2, K, early_stopping=early)
        after = st.arrays()
        for name in ("pool_seq", "pool_logprob", "pool_rank", "pool_len", "pool_ins"):
            assert torch.equal(after[name][0], before[name][0]), name
        assert torch.equal(bits(after["scores1"][0]), bits(before["scores0"][0])) and torch.equal(after["hist1"][0], before["hist0"][0])
        assert st.tok.view(K, 2)[:, 0].tolist() == [SEP] * K and st.parent.view(K, 2)[:, 0].tolist() == [0, 2] and not st.active[:, 0].any()
        assert st.active[:, 1].all()
    # a full pool whose worst entry an open beam can still beat: done only with early_stopping
    for early in (False, True):
        st = full_pool([-5.0, -6.0], K, L_)
        step(st, one_hot_rows(1, V_, [(0, 5, -1.0), (0, 6, -2.0), (0, 7, -3.0), (0, 4, -4.0)]), 0, 1, early_stopping=early)
        assert st.done.tolist() == [int(early)]


def test_the_last_step_pools_open_hypotheses():
    K, V_, L_ = 2, 8, 3
    st = decode.PoolState(1, K, L_, 0.0, "cpu", SEP)
    st.hist[0][0] = torch.tensor([[4, 5, 0], [4, 6, 0]])
    st.scores[0][0] = torch.tensor([-1.0, -2.0])
    z = one_hot_rows(2, V_, [(0, 7, -0.5), (0, SEP, -1.0), (1, 7, -0.25), (1, 3, -9.0)])
    step(st, z, 2, K)
    # rank order: [4 5 7] -1.5, [4 5 SEP] -2 (rank 1 < K: offered, the pool is full and -2 < -1.5 ... -2.25), [4 6 7] -2.25
    assert st.pool_seq[0].tolist() == [[4, 5, 7], [4, 5, SEP]] and st.pool_len.tolist() == [[3, 3]] and st.done.tolist() == [1]
    assert st.pool_logprob.tolist() == [[-1.5, -2.0]] and not st.active.any()


# ------------------------------------------------------------------------------------------------ the argument checks
def test_argument_checks():
    z = torch.zeros((1, 16))
    for kw in (dict(beam=0), dict(beam=9), dict(n_best=0), dict(n_best=4), dict(max_len=0), dict(max_len=513)):
        args = dict(b=1, beam=3, max_len=4, n_best=1)
        args.update(kw)
        with pytest.raises(ValueError):
            decode.decode_beam_pool_host([z] * 4, args["b"], args["beam"], args["max_len"], None, None, args["n_best"], eos=SEP)
    with pytest.raises(ValueError, match="2 \\* beam"):
        decode.decode_beam_pool_host([torch.zeros((3, 5))] * 4, 1, 3, 4, eos=SEP)                 # V = 5 < 2 K
    with pytest.raises(ValueError, match="SEP"):
        decode.decode_beam_pool_host([z] * 4, 1, 3, 4, eos=16)
    st = decode.PoolState(1, 3, 4, 0.0, "cpu", SEP)
    for t, cur in ((4, 3), (-1, 3), (0, 0), (0, 4)):
        with pytest.raises(ValueError):
            decode.beam_pool_step_host(torch.zeros((max(cur, 1), 16)), torch.zeros(max(cur, 1)), st, t, cur)
    with pytest.raises(ValueError):
        decode.beam_pool_step_host(torch.zeros((2, 16)), torch.zeros(2), st, 0, 1)               # rows != b * cur
    with pytest.raises(ValueError):                                                              # an answer set excludes the logits rules
        decode.decode_beam_pool_host([z] * 4, 1, 3, 4, decode.Constraints(min_length=2), decode.AnswerSet([[5]]), eos=SEP)
    # the device wrapper has no torch path: host tensors are refused
    from valor_amd import lib
    with pytest.raises((ValueError, lib.ValorHipError)):
        decode.beam_pool_step(z, torch.zeros(1), st, 0, 1)
    assert decode.inv_length_table(4, 1.0).tolist() == [1.0, 1.0, 0.5, float(f32(1 / 3)), 0.25]
    assert decode.inv_length_table(3, 0.0).tolist() == [1.0] * 4
