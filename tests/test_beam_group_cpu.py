"""The law of the diverse (group) beam search with finished-hypothesis pools, on the host (no GPU): decode.decode_beam_pool_host with
num_beam_groups against an independent plain-Python search (whole hypotheses in lists, one object per group, numpy fp32 scalars), the
two identities (one group == the pool law, penalty 0 == independent pool searches of beam K / G), the hand-derived rules of one step
(beam_group_step_host: the penalty and its multiplicity, ties, [SEP], done groups, the bound), the result order and the argument checks."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from valor_amd import decode  # noqa: E402
import test_beam_pool_cpu as C  # noqa: E402  (the random scripts of the pool law's tests)

INF = float("inf")
SEP = C.SEP
f32 = np.float32
bits = C.bits


def np_bits(x):
    return int(np.array([x], dtype=f32).view(np.int32)[0])


# ------------------------------------------------------------------------------------------------ an independent search, for clarity
class Group:
    """one beam group of one sample: its open hypotheses (best-first list; the index is the slot within the group), its pool"""

    def __init__(self, g, Kg):
        self.g, self.Kg, self.beams, self.pool, self.inserted, self.done = g, Kg, [(f32(0.0), [])], [], 0, False

    def offer(self, words, length, c, inv):
        rank = f32(c * inv[length])
        entry = dict(words=words, length=length, rank=rank, logp=c, ins=self.inserted, group=self.g)
        if len(self.pool) < self.Kg:
            self.pool.append(entry)
            self.inserted += 1
        else:
            worst = min(self.pool, key=lambda e: (float(e["rank"]), -e["ins"]))
            if rank > worst["rank"]:
                self.pool[self.pool.index(worst)] = entry
                self.inserted += 1

    def step(self, t, s, b, row, lse, taken_words, pen, inv, L_, alpha, early, eos):
        """row(r) / lse(r): the logits and the log-sum-exp of decoder row r; taken_words: what earlier groups' new open slots took"""
        Kg, V_ = self.Kg, len(row(0))
        cands = []
        for j, (cj, _) in enumerate(self.beams):
            k = 0 if t == 0 else self.g * Kg + j                     # the slot within the sample: at step 0 the one row of slot 0
            r = k * b + s
            z = row(r)
            for w in range(V_):
                c = f32(cj + f32(z[w] - lse(r)))
                a = f32(c - pen[taken_words.count(w)])
                if a > -INF:
                    cands.append((a, k * V_ + w, c, j, w))
        cands.sort(key=lambda x: (-float(x[0]), x[1]))
        new = []
        for rho, (_, _, c, j, w) in enumerate(cands[:2 * Kg]):
            if len(new) == Kg:
                break
            words = self.beams[j][1] + [w]
            if w == eos:
                if rho < Kg:
                    self.offer(words, t + 1, c, inv)
                continue
            new.append((c, words))
            if t == L_ - 1:
                self.offer(words, L_, c, inv)
        self.beams = new
        if t == L_ - 1 or not new:
            self.done = True
        elif len(self.pool) == Kg:
            worst = min(float(e["rank"]) for e in self.pool)
            top = max(c for c, _ in new)
            self.done = early or worst >= float(f32(top * inv[L_ if alpha > 0 else t + 2]))
        return [words[-1] for _, words in new]


def plain_group_search(script, b, K, G, L_, alpha, early, eos, lam, n):
    """Diverse beam search, one sample at a time. script[t]: logits [>= K * b, V_], rows beam-major. -> per sample the n first of the
    result order as (words padded with eos, length, rank, logP, group), or None for a missing entry."""
    Kg = K // G
    inv = [f32(1.0)] + [f32(1.0 / float(l) ** alpha) for l in range(1, L_ + 1)]
    pen = [f32(lam * m) for m in range(K + 1)]
    lses = [C.lse_rows(z).numpy() for z in script]
    rows = [z.numpy() for z in script]
    out = []
    for s in range(b):
        groups = [Group(g, Kg) for g in range(G)]
        for t in range(L_):
            taken = []
            for grp in groups:
                if not grp.done:
                    taken += grp.step(t, s, b, lambda r: rows[t][r], lambda r: lses[t][r], list(taken), pen, inv, L_, alpha, early, eos)
            if all(grp.done for grp in groups):
                break
        placed = []
        for grp in groups:
            best = sorted(grp.pool, key=lambda e: (-float(e["rank"]), e["ins"]))
            for p in range(Kg):
                e = best[p] if p < len(best) else None
                placed.append((p, INF if e is None else -float(e["rank"]), grp.g, e))
        placed.sort(key=lambda x: x[:3])
        out.append([None if e is None else (e["words"] + [eos] * (L_ - len(e["words"])), e["length"], e["rank"], e["logp"], e["group"])
                    for _, _, _, e in placed[:n]])
    return out


@pytest.mark.parametrize("K,G", [(2, 2), (4, 2), (6, 3), (8, 4), (8, 8)])
@pytest.mark.parametrize("alpha", [0.0, 1.0, -1.0, 0.7])
@pytest.mark.parametrize("early", [False, True])
def test_host_law_equals_an_independent_search(K, G, alpha, early):
    b, L_, V_, eos = 2, 7, 20, 2
    c = decode.Constraints(length_penalty=alpha) if alpha else None
    differed = False
    for lam in (0.0, 0.5, 16.0):
        for seed in (0, 1):
            script = C.random_script(seed * 10 + K, b, K, L_, V_, eos)
            seqs, rank, logp, length, group = decode.decode_beam_pool_host(script, b, K, L_, c, None, K, early, eos=eos, num_beam_groups=G,
                                                                           diversity_penalty=lam)
            want = plain_group_search(script, b, K, G, L_, alpha, early, eos, lam, K)
            assert seqs.shape == (b, K, L_) and rank.shape == logp.shape == length.shape == group.shape == (b, K)
            for s in range(b):
                for j, e in enumerate(want[s]):
                    assert e is not None
                    words, ln, rk, lp, g = e
                    assert seqs[s, j].tolist() == words and int(length[s, j]) == ln and int(group[s, j]) == g, (lam, seed, s, j)
                    assert bits(rank[s, j:j + 1]).item() == np_bits(rk) and bits(logp[s, j:j + 1]).item() == np_bits(lp), (lam, seed, s, j)
                if lam:
                    differed |= len({tuple(r) for r in seqs[s].tolist()}) > K // G
    assert differed                                                  # a penalty makes the groups differ (penalty 0: G copies of one search)


# ------------------------------------------------------------------------------------------------ the two identities
@pytest.mark.parametrize("K", [1, 3, 8])
def test_one_group_is_the_pool_law_step_by_step(K):
    b, L_, V_, eos = 3, 7, 20, 2
    for alpha, early, seed in ((0.0, False, 0), (0.7, False, 1), (-1.0, True, 2)):
        script = C.random_script(seed * 10 + K, b, K, L_, V_, eos)
        pool = decode.PoolState(b, K, L_, alpha, "cpu", eos)
        grp = decode.GroupPoolState(b, K, 1, L_, alpha, "cpu", eos)
        for t in range(L_):
            cur = 1 if t == 0 else K
            z = script[t][:b * cur]
            decode.beam_pool_step_host(z, C.lse_rows(z), pool, t, cur, early)
            decode.beam_group_step_host(z, C.lse_rows(z), grp, t, cur, early)
            pa, ga = pool.arrays(), grp.arrays()
            for name in pa:
                x, y = pa[name], ga[name].reshape(pa[name].shape)
                assert torch.equal(bits(x), bits(y)) if x.dtype == torch.float32 else torch.equal(x, y), (name, t)
            assert torch.equal(grp.gdone[:, 0], grp.done)
        assert grp.done.all()
        for x, y in zip(pool.result(K), grp.result(K)[:4]):
            assert torch.equal(x, y)
        assert (grp.result(K)[4] == 0).all()


@pytest.mark.parametrize("K,G", [(4, 2), (6, 3), (8, 4), (8, 8)])
def test_penalty_zero_makes_every_group_an_independent_pool_search(K, G):
    b, L_, V_, eos, Kg = 3, 7, 20, 2, K // G
    for alpha, early, seed in ((0.0, False, 0), (1.0, True, 1)):
        script = C.random_script(seed * 10 + K, b, K, L_, V_, eos)
        grp = decode.GroupPoolState(b, K, G, L_, alpha, "cpu", eos, diversity_penalty=0.0)
        pools = [decode.PoolState(b, Kg, L_, alpha, "cpu", eos) for _ in range(G)]
        for t in range(L_):
            cur = 1 if t == 0 else K
            z = script[t][:b * cur]
            decode.beam_group_step_host(z, C.lse_rows(z), grp, t, cur, early)
            o = (t + 1) % 2
            for g, pool in enumerate(pools):
                lo = g * Kg
                zg = z if t == 0 else z[lo * b:(lo + Kg) * b]            # the rows of the group's slots, beam-major
                decode.beam_pool_step_host(zg, C.lse_rows(zg), pool, t, 1 if t == 0 else Kg, early)
                assert torch.equal(bits(grp.scores[o][:, lo:lo + Kg]), bits(pool.scores[o])), (t, g)
                assert torch.equal(grp.hist[o][:, lo:lo + Kg], pool.hist[o])
                for name in ("pool_seq", "pool_len", "pool_ins"):
                    assert torch.equal(getattr(grp, name)[:, lo:lo + Kg], getattr(pool, name)), (name, t, g)
                for name in ("pool_logprob", "pool_rank"):
                    assert torch.equal(bits(getattr(grp, name)[:, lo:lo + Kg]), bits(getattr(pool, name))), (name, t, g)
                assert torch.equal(grp.pool_cnt[:, g], pool.pool_cnt) and torch.equal(grp.gdone[:, g], pool.done)
                assert torch.equal(grp.tok.view(K, b)[lo:lo + Kg], pool.tok.view(Kg, b))
                assert torch.equal(grp.active[lo:lo + Kg], pool.active)
                # a parent is a decoder row: the group's slots sit lo rows of b further on, except the step-0 children of slot 0
                from_slot0 = (pool.scores[o] > -INF).t() & (t == 0)
                want = torch.where(from_slot0, pool.parent.view(Kg, b), pool.parent.view(Kg, b) + lo * b)
                assert torch.equal(grp.parent.view(K, b)[lo:lo + Kg], want), (t, g)
            assert torch.equal(grp.done, torch.stack([p.done for p in pools], 1).all(1).to(torch.uint8))
    # a decoder's rows depend on the words alone (here: every slot reads the same row), so all groups return the same thing
    script = [z[:b].repeat(K, 1) for z in C.random_script(K, b, K, L_, V_, eos)]
    seqs, rank, logp, length, group = decode.decode_beam_pool_host(script, b, K, L_, None, None, K, eos=eos, num_beam_groups=G)
    assert group[:, :G].tolist() == [list(range(G))] * b
    for g in range(1, G):
        assert torch.equal(seqs[:, 0::G], seqs[:, g::G]) and torch.equal(bits(logp[:, 0::G]), bits(logp[:, g::G]))


# ------------------------------------------------------------------------------------------------ the rules of one step, by hand
def state(K, G, L_, lam, b=1, alpha=0.0):
    return decode.GroupPoolState(b, K, G, L_, alpha, "cpu", SEP, diversity_penalty=lam)


def step(st, z, t, cur, **kw):
    return decode.beam_group_step_host(z, torch.zeros(z.shape[0]), st, t, cur, **kw)      # lse 0: the logits are the log-probabilities


def test_step_0_by_hand_and_the_scores_stay_unpenalised():
    """K = 4, G = 2, one row, [SEP] at -inf, the logits spread over less than the penalty 16: group 0 takes the two best words (9, 7);
    group 1 sees them at c - 16, below every other word, and takes the third and fourth (5, 11); all carry their own c"""
    z = torch.full((1, 12), -6.0)
    z[0, SEP] = -INF
    z[0, 9], z[0, 7], z[0, 5], z[0, 11] = -0.5, -1.0, -1.5, -2.0
    st = state(4, 2, 5, 16.0)
    step(st, z, 0, 1)
    assert st.tok.tolist() == [9, 7, 5, 11] and st.parent.tolist() == [0, 0, 0, 0]
    assert st.scores[1].tolist() == [[-0.5, -1.0, -1.5, -2.0]]
    assert st.hist[1][0, :, 0].tolist() == [9, 7, 5, 11] and st.active.all() and not st.gdone.any() and not st.done.any()
    assert st.pool_cnt.tolist() == [[[0, 0], [0, 0]]]
    # without the penalty both groups take the same two
    st = state(4, 2, 5, 0.0)
    step(st, z, 0, 1)
    assert st.tok.tolist() == [9, 7, 9, 7] and st.scores[1].tolist() == [[-0.5, -1.0, -0.5, -1.0]]
    # a penalty smaller than the gap reorders nothing but is still not carried: 9 at -0.5 - 0.75 = -1.25 lies between 7 and 5
    st = state(4, 2, 5, 0.75)
    step(st, z, 0, 1)
    assert st.tok.tolist() == [9, 7, 9, 5] and st.scores[1].tolist() == [[-0.5, -1.0, -0.5, -1.5]]       # keys -1.25 (9), -1.5 (5), -1.75 (7)


def test_two_earlier_slots_with_one_word_give_pen_2():
    """K = G = 3, penalty 2. Group 0 takes 5 (0). Group 1: 5 at 0 - 2 = -2 still beats 6 (-3): it takes 5 too. Group 2: two slots hold
    5, its key is 0 - pen[2] = -4, below 6 (-3) and 7 (-3.9); with pen[1] it would have been taken again"""
    z = torch.full((1, 8), -INF)
    z[0, 5], z[0, 6], z[0, 7] = 0.0, -3.0, -3.9
    st = state(3, 3, 4, 2.0)
    assert st.pen.tolist() == [0.0, 2.0, 4.0, 6.0]
    step(st, z, 0, 1)
    assert st.tok.tolist() == [5, 5, 6] and st.scores[1].tolist() == [[0.0, 0.0, -3.0]]
    # the table is the fp64 product rounded once
    assert decode.diversity_table(3, 0.1).tolist() == [0.0, float(f32(0.1)), float(f32(0.2)), float(f32(0.1 * 3))]


def test_a_penalised_word_tying_an_unpenalised_one_resolves_by_index():
    for other, want in ((3, 3), (9, 5)):                             # 5 at 0 - 1 == -1 == the other word: the lower index wins
        z = torch.full((1, 12), -INF)
        z[0, 5], z[0, other] = 0.0, -1.0
        st = state(2, 2, 4, 1.0)
        step(st, z, 0, 1)
        assert st.tok.tolist() == [5, want], other
        assert st.scores[1].tolist() == [[0.0, 0.0 if want == 5 else -1.0]]


def test_sep_is_never_penalised():
    """both groups see [SEP] as their best candidate: each pools it at its own c, under any penalty, and the word that group 0 took (5) is
    what the penalty moves"""
    z = torch.full((1, 12), -INF)
    z[0, SEP], z[0, 5], z[0, 6] = -0.25, -0.5, -0.75
    st = state(2, 2, 4, 16.0)
    step(st, z, 0, 1)
    assert st.pool_cnt.tolist() == [[[1, 1], [1, 1]]] and st.pool_logprob.tolist() == [[-0.25, -0.25]]
    assert st.pool_len.tolist() == [[1, 1]] and (st.pool_seq == SEP).all()
    assert st.tok.tolist() == [5, 6] and st.scores[1].tolist() == [[-0.5, -0.75]]


def test_done_groups_are_frozen_and_lend_no_words():
    K, G, L_, V_ = 4, 2, 4, 12
    st = state(K, G, L_, 16.0, b=2)
    st.scores[1][:] = torch.tensor([[-1.0, -2.0, -1.5, -2.5]] * 2)
    st.hist[1][:, :, 0] = torch.tensor([[5, 6, 7, 8]] * 2)
    st.gdone[0, 0] = 1                                               # sample 0: group 0 done; sample 1: nobody
    z = torch.full((K * 2, V_), -INF)
    z[:, 9], z[:, 10], z[:, 3] = -0.125, -0.25, -5.0
    step(st, z, 1, K)
    # sample 0, group 0: frozen (scores and words as they were, tok [SEP], parent the row itself, inactive); group 1 takes the best
    # word 9 of both its slots as if group 0 were not there
    assert st.scores[0][0].tolist() == [-1.0, -2.0, -1.625, -1.75] and st.hist[0][0, :2].tolist() == [[5, 0, 0, 0], [6, 0, 0, 0]]
    assert st.tok.view(K, 2)[:, 0].tolist() == [SEP, SEP, 9, 10] and st.parent.view(K, 2)[:, 0].tolist() == [0, 2, 4, 4]
    assert st.active[:, 0].tolist() == [0, 0, 1, 1] and st.gdone[0].tolist() == [1, 0] and st.done.tolist() == [0, 0]
    # sample 1: group 0 takes 9 and 10 of its slot 0, group 1 pays 16 for both and takes word 3 twice
    assert st.tok.view(K, 2)[:, 1].tolist() == [9, 10, 3, 3] and st.scores[0][1].tolist() == [-1.125, -1.25, -6.5, -7.5]
    # sample 0 goes on with one group until that is done too; then done[s]
    z[:, :] = -INF
    z[:, SEP], z[:, 9] = -0.125, -4.0
    step(st, z, 2, K, early_stopping=True)
    assert st.pool_cnt[0].tolist() == [[0, 0], [2, 2]] and st.gdone[0].tolist() == [1, 1] and st.done.tolist() == [1, 1]
    assert not st.active.any()
    # the last step pools every open hypothesis of every group that is not done
    st = state(K, G, 3, 16.0)
    st.scores[0][0] = torch.tensor([-1.0, -2.0, -1.5, -2.5])
    st.hist[0][0, :, :2] = torch.tensor([[5, 5], [6, 6], [7, 7], [8, 8]])
    z = torch.full((K, V_), -INF)
    z[:, 9], z[:, 10] = -0.125, -3.0
    step(st, z, 2, K)
    assert st.done.tolist() == [1] and st.gdone.all() and st.pool_cnt.tolist() == [[[2, 2], [2, 2]]] and not st.active.any()
    assert st.pool_seq[0].tolist() == [[5, 5, 9], [6, 6, 9], [7, 7, 10], [8, 8, 10]] and st.pool_len.tolist() == [[3] * 4]
    assert st.pool_logprob.tolist() == [[-1.125, -2.125, -4.5, -5.5]]


def test_the_bound_uses_the_largest_new_score_of_the_group():
    """K = 4, G = 2, penalty 1.5. Group 0 takes 5 (-0.1) and 6 (-0.2). Group 1's keys: 7 at -1.0, 5 at -0.1 - 1.5 = -1.6, 6 at -1.7:
    its new slot 0 holds 7 (-1.0) and its slot 1 holds 5 (-0.1). Its pool is full, worst rank -0.5: slot 0 alone would end the group
    (-0.5 >= -1.0), the largest new score does not (-0.5 < -0.1)"""
    z = torch.full((1, 12), -INF)
    z[0, 5], z[0, 6], z[0, 7] = -0.1, -0.2, -1.0
    for worst, want in ((-0.5, 0), (-0.05, 1)):
        st = state(4, 2, 6, 1.5)
        st.pool_rank[0, 2:] = st.pool_logprob[0, 2:] = torch.tensor([worst, -0.04])
        st.pool_ins[0, 2:], st.pool_len[0, 2:] = torch.tensor([0, 1], dtype=torch.int32), 1
        st.pool_cnt[0, 1] = 2
        step(st, z, 0, 1)
        assert st.tok.tolist() == [5, 6, 7, 5] and st.scores[1][0, 2:].tolist() == [-1.0, pytest.approx(-0.1)]
        assert st.gdone.tolist() == [[0, want]] and st.done.tolist() == [0]
        assert st.active[:, 0].tolist() == [1, 1, 1 - want, 1 - want]


# ------------------------------------------------------------------------------------------------ the interface
def test_result_order_and_groups():
    st = state(4, 2, 3, 1.0)
    # group 0 holds ranks (-3, -1), group 1 (-2, -2) with the later entry inserted first
    st.pool_rank[0] = st.pool_logprob[0] = torch.tensor([-3.0, -1.0, -2.0, -2.0])
    st.pool_ins[0] = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    st.pool_len[0] = torch.tensor([1, 2, 3, 1], dtype=torch.int32)
    st.pool_seq[0, :, 0] = torch.tensor([20, 21, 22, 23])
    seqs, rank, logp, length, group = st.result(4)
    # place 0: group 0's -1 before group 1's -2 (the older of the two equal ones); place 1: group 1's -2 before group 0's -3
    assert seqs[0, :, 0].tolist() == [21, 23, 22, 20] and rank.tolist() == [[-1.0, -2.0, -2.0, -3.0]] and group.tolist() == [[0, 1, 1, 0]]
    assert length.tolist() == [[2, 1, 3, 1]] and group.dtype == torch.int64
    assert st.result(2)[4].tolist() == [[0, 1]]                      # the first G: one hypothesis per group
    st.pool_rank[0, 1] = -2.0                                        # equal scores at one place: by group index
    assert st.result(2)[0][0, :, 0].tolist() == [21, 23]
    st.pool_rank[0, 1] = -2.5
    assert st.result(2)[0][0, :, 0].tolist() == [23, 21]


def test_argument_checks():
    z = torch.zeros((4, 16))
    host = lambda **kw: decode.decode_beam_pool_host([z] * 4, 1, kw.pop("beam", 4), 4, None, None, kw.pop("n_best", 1), eos=SEP, **kw)
    for kw in (dict(num_beam_groups=3), dict(num_beam_groups=0), dict(num_beam_groups=8), dict(num_beam_groups=2, diversity_penalty=-0.5),
               dict(num_beam_groups=2, diversity_penalty=INF), dict(num_beam_groups=2, diversity_penalty=float("nan")),
               dict(num_beam_groups=1, diversity_penalty=0.5), dict(num_beam_groups=2, n_best=5), dict(num_beam_groups=1.5)):
        with pytest.raises(ValueError):
            host(**kw)
    assert len(host(num_beam_groups=2, diversity_penalty=0.5, n_best=4)) == 5 and len(host()) == 4
    with pytest.raises(ValueError):
        decode.GroupPoolState(1, 4, 3, 4)
    st = state(4, 2, 4, 1.0)
    for t, cur, V_ in ((0, 2, 16), (0, 3, 16), (0, 0, 16), (4, 4, 16), (0, 1, 3)):          # cur not in {1, K}; t; V < 2 Kg
        with pytest.raises(ValueError):
            decode.beam_group_step_host(torch.zeros((max(cur, 1), V_)), torch.zeros(max(cur, 1)), st, t, cur)
    with pytest.raises(ValueError):
        decode.beam_group_step_host(torch.zeros((2, 16)), torch.zeros(2), st, 0, 1)           # rows != b * cur
    from valor_amd import lib
    with pytest.raises((ValueError, lib.ValorHipError)):                                     # no torch path: host tensors are refused
        decode.beam_group_step(torch.zeros((1, 16)), torch.zeros(1), st, 0, 1)
    assert "valor_beam_group_step" in lib.SIGNATURES


def test_generate_arguments_and_model_options():
    model = types.SimpleNamespace(opts={"generation_num_beam_groups": 2, "generation_diversity_penalty": 0.5})
    plain = types.SimpleNamespace(opts={})
    g = decode._beam_groups
    assert g("generate_cap", model, "pool", 4, None, None) == (2, 0.5)              # the options are the defaults ...
    assert g("generate_cap", model, "pool", 4, 4, 1.0) == (4, 1.0)                  # ... the call's arguments win ...
    assert g("generate_cap", model, "reference", 1, None, None, False) == (1, 0.0)  # ... they do not apply to a call without a beam search
    assert g("generate_cap", model, "reference", 4, 1, 0.0) == (1, 0.0)             # ... and a searching call can switch them off
    with pytest.raises(ValueError, match="options"):                                # but groups asked for under the reference rule: refused
        g("generate_cap", model, "reference", 4, None, None)
    with pytest.raises(ValueError, match="options"):
        g("generate_cap", model, "reference", 4, 1, None)                           # (the option's penalty is still on)
    assert g("generate_cap", plain, "pool", 4, None, None) == (1, 0.0)
    assert g("generate_cap", plain, "reference", 4, 1, 0.0) == (1, 0.0)
    for rule, beam, G, lam in (("reference", 4, 2, None), ("reference", 4, None, 0.5), ("pool", 4, 3, 0.5), ("pool", 4, 2, -1.0),
                               ("pool", 4, 2, INF), ("pool", 4, 1, 0.5), ("pool", 3, None, None)):
        with pytest.raises(ValueError):
            g("generate_cap", model if G is None and beam == 3 else plain, rule, beam, G, lam)
    import inspect
    for fn in (decode.generate_cap, decode.generate_qa):
        p = inspect.signature(fn).parameters
        assert p["num_beam_groups"].default is None and p["diversity_penalty"].default is None
    # the named outputs: sequence_groups_* comes beside the others under groups only
    five = (torch.zeros((2, 2, 3), dtype=torch.int64), torch.zeros((2, 2)), torch.zeros((2, 2)), torch.zeros((2, 2)), torch.tensor([[0, 1]] * 2))
    out = decode._named_pool("generated_sequences_", {"tva": five})
    assert out["sequence_groups_t_va"].tolist() == [0, 1, 0, 1] and out["sequence_groups_t_va"].dtype == torch.int64
    assert set(decode._named_pool("generated_sequences_", {"tva": five[:4]})) == {"generated_sequences_t_va", "sequence_scores_t_va",
                                                                                  "sequence_logprobs_t_va"}
