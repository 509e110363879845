"""Exact ranking of a closed answer set, the host side: AnswerSet.levels() (the breadth-first plan of the level-batched pass),
decode.trie_level_host (the law of valor_trie_score_level) level by level against an fp64 sum of log-softmax terms, the row counts
that are the reason the feature exists, and the refusals that need no device."""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, V, SEP = 3, 40, 2                        # the scripted geometry of tests/test_answer_set_decode_gpu.py: [SEP] is column 2
CANDS = [[7, 8, 9], [7, 8], [7, 5], [30], [10, 11, 12, 13], [7, 8]]
#         shared prefixes (7 ..), a terminal node with children ([7 8] under [7 8 9]), a duplicate ([7 8] twice), a candidate that is a
#         prefix of another ([7 8] of [7 8 9])


@pytest.fixture
def sep(monkeypatch):
    from valor_amd import decode
    monkeypatch.setattr(decode, "EOS", SEP)
    return SEP


def test_levels_is_the_trie_in_breadth_first_order():
    from valor_amd import decode
    a = decode.AnswerSet(CANDS)
    lv = a.levels()
    assert lv is a.levels()                                                       # cached on the set
    N = a.n_nodes
    order = lv.order.tolist()
    assert len(order) == N == 10 and sorted(order) == list(range(N))             # root, 7, 30, 10, 7-8, 7-5, 10-11, 7-8-9, 10-11-12, ..-13
    assert lv.depth_max == 4 == a.max_len and len(lv.level_ptr) == lv.depth_max + 2
    assert [lv.level_ptr[d + 1] - lv.level_ptr[d] for d in range(5)] == [1, 3, 3, 2, 1] and lv.width == 3
    assert order[0] == int(a.root[0]) and int(lv.parent[order[0]]) == -1 and int(lv.token[order[0]]) == decode.BOS
    where = {n: i for i, n in enumerate(order)}
    for d in range(lv.depth_max + 1):
        for n in order[lv.level_ptr[d]:lv.level_ptr[d + 1]]:
            assert int(lv.depth[n]) == d                                          # every node once, at its depth
            if d:
                p = int(lv.parent[n])
                assert where[p] < where[n] and int(lv.depth[p]) == d - 1          # parents precede children
                assert a._step(p, int(lv.token[n])) == n                          # ... along the node's token
            anc = lv.anc[n].tolist()
            assert anc[d] == n and anc[d + 1:] == [-1] * (lv.depth_max - d)
            assert all(int(lv.parent[anc[j + 1]]) == anc[j] for j in range(d))
    cn = lv.cand_node.tolist()
    assert len(cn) == len(CANDS) and cn[1] == cn[5] and len(set(cn)) == 5         # the duplicates share a node
    for c, n in zip(CANDS, cn):
        assert int(a.terminal[n]) == 1 and int(lv.depth[n]) == len(c)
        assert [int(lv.token[x]) for x in lv.anc[n].tolist()[1:len(c) + 1]] == c
    assert int(a.child_ptr[cn[1] + 1] - a.child_ptr[cn[1]]) == 1                  # the terminal node [7 8] has a child
    per = decode.AnswerSet([[[7]], [[8]]], per_sample=True)
    with pytest.raises(ValueError, match="per-sample"):
        per.levels()


def test_trie_level_host_level_by_level_against_fp64(sep):
    """scripted fp32 logits, one row per (node, sample); the candidates' scores after the last level against a plain fp64 sum of
    log-softmax terms. The band, per candidate of L tokens, is (L + 1) * 208 * 2^-24: with |lse| < 8, |term| < 16 and |partial sum| <
    128 (asserted), a term carries the error of torch's fp32 log-sum-exp (taken as <= 4 ulp: 8 * 2^-24 * 8), the rounding of the
    subtraction (2^-24 * 16) and the rounding of the addition into the running sum (2^-24 * 128)."""
    from valor_amd import decode
    a = decode.AnswerSet(CANDS)
    lv = a.levels()
    N = a.n_nodes
    g = torch.Generator().manual_seed(3)
    z = torch.randn((N, B, V), generator=g) * 2.0                                 # z[node, sample]: the step's logits after the node's prefix
    lse = torch.logsumexp(z, 2)
    ns, fin = torch.zeros(N * B), torch.full((N * B,), float("nan"))
    for d in range(lv.depth_max + 1):
        nodes = lv.order[lv.level_ptr[d]:lv.level_ptr[d + 1]]
        rows = z[nodes.long()].reshape(-1, V)
        given, copy = ns, ns.clone()
        ns, fin = decode.trie_level_host(rows, lse[nodes.long()].reshape(-1), nodes, B, a, sep, ns, fin)
        assert torch.equal(given, copy) and ns is not given and ns.dtype == fin.dtype == torch.float32      # the inputs are not modified
    got = fin.view(N, B)[lv.cand_node].t()                                        # [B, C]
    assert not torch.isnan(got).any()
    assert torch.isnan(fin.view(N, B)[~a.terminal.bool()]).all()                  # a node where no candidate ends has no final score
    assert float(lse.abs().max()) < 8
    lp = torch.log_softmax(z.double(), 2)
    for c, cand in enumerate(CANDS):
        path = lv.anc[lv.cand_node[c]].tolist()[:len(cand) + 1]
        for s in range(B):
            terms = [float(lp[n, s, w]) for n, w in zip(path, cand + [sep])]
            assert max(abs(t) for t in terms) < 16 and abs(sum(terms)) < 128
            band = (len(cand) + 1) * 208 * 2.0 ** -24
            assert abs(float(got[s, c]) - sum(terms)) <= band, (c, s, float(got[s, c]), sum(terms))
    assert torch.equal(got[:, 1], got[:, 5])                                      # duplicates: equal scores
    # lse=None takes torch's fp32 log-sum-exp: the same numbers here
    ns2, fin2 = decode.trie_level_host(z[lv.order[:1].long()].reshape(-1, V), None, lv.order[:1], B, a, sep, torch.zeros(N * B),
                                       torch.zeros(N * B))
    kids = lv.order[lv.level_ptr[1]:lv.level_ptr[2]].long()
    assert torch.equal(ns2.view(N, B)[kids], ns.view(N, B)[kids])
    with pytest.raises(ValueError, match="rows"):
        decode.trie_level_host(z[0], None, lv.order[:2], B, a, sep, ns, fin)


def test_the_tree_runs_less_than_half_the_rows_of_forced_decoding():
    """the reason the feature exists: for a 3129-answer set of 1..4 tokens (the VQAv2 size) score_candidates runs C * (Lmax + 1) decoder
    rows per sample, the tree pass one per trie node"""
    from valor_amd import decode, synth
    cands = synth.make_answer_set(3129, 30522, seed=1)
    assert len(cands) == 3129 and len({tuple(c) for c in cands}) == 3129
    assert {len(c) for c in cands} == {1, 2, 3, 4}
    a = decode.AnswerSet(cands, vocab=30522)
    lv = a.levels()
    forced = len(cands) * (a.max_len + 1)
    print(f"decoder rows per sample: tree {a.n_nodes}, forced decoding {forced}")
    assert forced == 15645 and a.n_nodes == 3849                                 # the two counts (seed 1)
    assert a.n_nodes < forced / 2
    assert a.n_nodes < forced / 3                                                 # ... with room to spare
    assert lv.level_ptr[-1] == a.n_nodes and lv.depth_max == 4


def test_entry_point_validates_its_arguments_without_a_device():
    """valor_trie_score_level returns VALOR_ERR_ARG (-1) before any launch; rows == 0 is a no-op"""
    import ctypes
    from valor_amd import lib
    so = lib.load()
    f = (ctypes.c_float * 64)()
    i = (ctypes.c_int32 * 8)()
    u = (ctypes.c_uint8 * 8)()
    p = ctypes.addressof

    def call(logits=p(f), ld=16, rows=4, V=16, b=2, level_node=p(i), eos=2, child_ptr=p(i), child_tok=p(i), child_node=p(i), terminal=p(u),
             n_nodes=4, n_edges=3, node_score=p(f), final=p(f)):
        return so.valor_trie_score_level(None, logits, ld, rows, V, b, level_node, None, None, eos, child_ptr, child_tok, child_node, terminal,
                                         n_nodes, n_edges, node_score, final)
    assert call(rows=0) == 0 and call(rows=0, logits=None) == 0
    for bad in (dict(logits=None), dict(level_node=None), dict(child_ptr=None), dict(terminal=None), dict(node_score=None), dict(final=None),
                dict(child_tok=None), dict(child_node=None), dict(ld=15), dict(V=0), dict(eos=16), dict(eos=-1), dict(b=0), dict(rows=-2),
                dict(rows=5), dict(rows=10), dict(n_nodes=0), dict(n_edges=-1)):
        assert call(**bad) == -1, bad


def test_refusals_need_no_device():
    from valor_amd import decode
    from valor_amd.evaluate import validate_qa
    per = decode.AnswerSet([[[7]], [[8]]], per_sample=True)
    with pytest.raises(ValueError, match="score_candidates"):
        decode.rank_candidates(None, {}, ["tv"], per)
    with pytest.raises(ValueError, match="no candidates"):
        decode.rank_candidates(None, {}, ["tv"], None)
    with pytest.raises(ValueError, match="k = 0"):
        decode.rank_candidates(None, {}, ["tv"], [[7], [8]], k=0)
    with pytest.raises(ValueError, match="k = 3"):
        decode.rank_candidates(None, {}, ["tv"], [[7], [8]], k=3)
    model = types.SimpleNamespace(opts=None)
    with pytest.raises(ValueError, match="needs candidates"):
        validate_qa(model, [], "qa%tv", answer_ranking="exact")
    with pytest.raises(ValueError, match="multiple_choice"):
        validate_qa(model, [], "qa%tv", answer_ranking="exact", multiple_choice=True)
    with pytest.raises(ValueError, match="multiple_choice"):
        validate_qa(model, [], "qa%tv", answer_ranking="exact", multiple_choice=True, candidates=[[7]])
    with pytest.raises(ValueError, match="answer_ranking"):
        validate_qa(model, [], "qa%tv", answer_ranking="beam", candidates=[[7]])
    with pytest.raises(ValueError, match="shared"):
        validate_qa(model, [], "qa%tv", answer_ranking="exact", candidates=per)
    with pytest.raises(ValueError, match="needs candidates"):                     # the option alone asks for it too
        validate_qa(types.SimpleNamespace(opts={"qa_answer_ranking": "exact"}), [], "qa%tv")
