"""valor_trie_constrain on the GPU against the host law (decode.trie_rows_host), bit for bit: V in {17, 1000, 30522} with ld = V (rows
that are not 16-byte aligned: the scalar path) and ld = V padded to 32 with a marker in the pad (the 16-byte path), R in {1, 5, 192},
nodes with 0, 1, 63, 64, 65 and 5000 children (the last is past the LDS staging), t in {0, 1, 5}, histories that leave the trie or hold
[SEP] / an id >= V / a negative id, shared and per-sample roots, the row-ordered history and the beam-major strides, active given and
null, a base pointer that is not 16-byte aligned; eager issue == one graph capture + replay."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

MARK = 123.25
SEP = 102
T = 5                                         # the longest history of the grid


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


_ZOO = {}


def zoo():
    """one shared set whose nodes have 0, 1, 63, 64, 65 and 5000 children: the root has 5000 (tokens 3..8 and 4994 others below 30000);
    3 is a leaf, 4 has one child, 5 / 6 / 7 have 63 / 64 / 65, 8 starts the chain 8 9 10 11 12 13 whose node 8-9 is also an end.
    Built once and shared (read-only) by the tests."""
    if "a" not in _ZOO:
        from valor_amd import decode
        g = torch.Generator().manual_seed(7)
        pool = torch.tensor([w for w in range(14, 30000) if w != SEP])
        others = pool[torch.randperm(pool.numel(), generator=g)[:4994]].tolist()
        fan = lambda n: pool[torch.randperm(pool.numel(), generator=g)[:n]].tolist()
        cands = [[3], [4, 11]] + [[5, w] for w in fan(63)] + [[6, w] for w in fan(64)] + [[7, w] for w in fan(65)]
        cands += [[8, 9, 10, 11, 12, 13], [8, 9]] + [[w] for w in others]
        a = decode.AnswerSet(cands)
        counts = sorted(set((a.child_ptr[1:] - a.child_ptr[:-1]).tolist()))
        assert counts == [0, 1, 63, 64, 65, 5000], counts                            # the condition of the tests
        _ZOO["a"], _ZOO["others"], _ZOO["cands"] = a, others, cands
    return _ZOO["a"]


def per_sample_set(b):
    """a set per sample: two to four short answers that share a first token, one sample with a 65-way node"""
    from valor_amd import decode
    sets = []
    for s in range(b):
        base = 3 + (s % 11)
        c = [[base], [base, 9], [base + 1, 9, 10, 11, 12]][: 2 + s % 2] + [[16, 5 + s % 3]]
        if s % 4 == 1:
            c += [[15, w] for w in range(200, 265)]
        sets.append(c)
    return decode.AnswerSet(sets, per_sample=True)


def histories(R, V, g):
    """int64 [R, T]: paths inside the zoo (to a leaf, through every fan-out, down the chain), paths that leave it, and rows with [SEP],
    an id >= V and a negative id; behind the scripted prefix the tokens are random"""
    a = zoo()
    others, cands = _ZOO["others"], _ZOO["cands"]
    paths = [[3], [4, 11], cands[2], cands[2 + 63], cands[2 + 63 + 64 + 64], [8, 9, 10, 11, 12], [8, 9], [8, 9, 10, 11, 13], [others[0]],
             [others[4993]], [max(others)], [min(others)], [SEP, 3], [3, SEP], [V + 3, 8], [8, V], [-1, 8], [29999 if 29999 not in others else 13],
             [5, 13], [8, 9, 10, 9], [2 ** 33 + 3]]
    h = torch.randint(1, 14, (R, T), generator=g)
    for r in range(R):
        p = paths[r % len(paths)] if r < 2 * len(paths) else None
        if p is not None:
            h[r, :len(p)] = torch.tensor(p)
    return h


def buffers(logits, dev, padded):
    """fp32 host rows [R, V] -> (storage, view [R, V]): ld = V (no pad; the rows start wherever R * V puts them) or V rounded up to
    32 with MARK in the pad columns"""
    R, V = logits.shape
    if not padded:
        buf = logits.to(dev).contiguous()
        return buf, buf
    ld = (V + 31) // 32 * 32
    buf = torch.full((R, ld), MARK, dtype=torch.float32, device=dev)
    buf[:, :V] = logits.to(dev)
    return buf, buf[:, :V]


def check(dev, a, logits, hist, t, eos, nb, active, padded, **kw):
    from valor_amd import decode, kernels as K
    R, V = logits.shape
    buf, view = buffers(logits, dev, padded)
    row_hist = kw.pop("row_hist", hist)
    K.trie_constrain(view, hist.to(dev) if t > 0 else None, t, eos, a.device(dev), None if active is None else active.to(dev), **kw)
    got = buf.cpu()
    want = decode.trie_rows_host(logits, row_hist, t, a, eos, nb, active)
    assert same_bits(got[:, :V], want), (V, R, t, padded, active is not None)
    if padded:
        assert (got[:, V:] == MARK).all(), (V, R, t)
    if active is not None:
        assert same_bits(got[:, :V][~active], logits[~active])
    return want


@pytest.mark.parametrize("V", [17, 1000, 30522])
def test_shared_set_equals_the_host_law_bit_for_bit(dev, V):
    a = zoo()
    eos = 2 if V < SEP else SEP
    g = torch.Generator().manual_seed(V)
    floored = kept = 0
    for R in (1, 5, 192):
        logits = torch.randn((R, V), generator=g)
        logits[:, V // 2] = float("nan")
        logits[0, min(8, V - 1)] = -0.0
        hist = histories(R, V, g)
        active = torch.rand(R, generator=g) < 0.7
        for t in (0, 1, 5):
            for padded in (False, True):
                for act in (None, active):
                    if R == 192 and V == 30522 and (act is None) != padded:          # (the largest shape: two of the four combinations)
                        continue
                    want = check(dev, a, logits, hist, t, eos, R, act, padded)
                    floored += int((want == decode_floor()).sum())
                    kept += int((want != decode_floor()).sum())
    assert floored > 0 and kept > 0


def decode_floor():
    from valor_amd import decode
    return decode.TRIE_FLOOR


def test_allowed_sets_of_the_zoo_rows(dev):
    """what the launch leaves open, spelled out for the scripted rows: the host law is the reference, this pins the law itself"""
    from valor_amd import kernels as K
    a = zoo()
    V, R = 30522, 21
    g = torch.Generator().manual_seed(5)
    hist = histories(R, V, g)
    logits = torch.randn((R, V), generator=g)
    open_cols = lambda t: [set(torch.nonzero(r != decode_floor()).view(-1).tolist())
                           for r in K.trie_constrain(logits.to(dev), hist.to(dev) if t else None, t, SEP, a.device(dev)).cpu()]
    o0, o1, o5 = open_cols(0), open_cols(1), open_cols(5)
    assert all(len(s) == 5000 and SEP not in s for s in o0)
    assert o1[0] == {SEP} and o1[1] == {11} and len(o1[2]) == 63 and len(o1[3]) == 64 and len(o1[4]) == 65 and o1[5] == {9}
    assert o1[12] == {SEP} and o1[14] == {SEP} and o1[16] == {SEP} and o1[20] == {SEP}   # [SEP], an id >= V, -1, 2^33 + 3: off the trie
    assert o1[8] == {SEP}                                                          # a one-token answer: the end
    assert o5[5] == {13} and o5[7] == {SEP} and o5[19] == {SEP}                       # 8 9 10 11 12 -> 13; 8 9 10 11 13 and 8 9 10 9: off the trie
    o2 = open_cols(2)
    assert o2[6] == {10, SEP} and o2[1] == {SEP} and o2[13] == {SEP}                   # 8 9: an end with a child; 4 11: a leaf; 3 [SEP]: off


@pytest.mark.parametrize("V", [17, 1000, 30522])
def test_per_sample_roots(dev, V):
    eos = 2 if V < SEP else SEP
    g = torch.Generator().manual_seed(V + 1)
    for b, beam in ((1, 1), (5, 1), (64, 3)):
        a = per_sample_set(b)
        R = b * beam
        logits = torch.randn((R, V), generator=g)
        hist = torch.randint(1, 14, (R, T), generator=g)
        for r in range(R):                                                          # half the rows follow one of their sample's answers
            c = a.candidates[r % b][r % a.counts[r % b]]
            if r % 2 == 0:
                hist[r, :len(c)] = torch.tensor(c)
        active = torch.rand(R, generator=g) < 0.7
        for t in (0, 1, 5):
            for padded in (False, True):
                check(dev, a, logits, hist, t, eos, b, active if padded else None, padded, b=b, hist_stride_s=T, hist_stride_k=b * T)


def test_history_through_the_beam_strides(dev):
    """beam-major rows r = k * b + s over words kept as [b, beam, max_len]: hist_stride_s = beam * max_len, hist_stride_k = max_len"""
    b, beam, max_len, V = 5, 3, 9, 1000
    g = torch.Generator().manual_seed(1)
    words = torch.randint(1, 14, (b, beam, max_len), generator=g)
    for a, shared in ((zoo(), True), (per_sample_set(b), False)):
        for s in range(b):
            for k in range(beam):
                c = (a.candidates[0][(s * beam + k) % 200] if shared else a.candidates[s][k % a.counts[s]])
                if (s + k) % 3:
                    words[s, k, :len(c)] = torch.tensor(c)
        row_hist = words.transpose(0, 1).reshape(b * beam, max_len)                 # row k * b + s reads words[s, k]
        logits = torch.randn((b * beam, V), generator=g)
        act = torch.ones(b * beam, dtype=torch.bool)
        act[[2, 7]] = False
        for t in (1, 2, 5):
            for padded in (False, True):
                check(dev, a, logits, words, t, SEP, b, act, padded, row_hist=row_hist, b=b, hist_stride_s=beam * max_len, hist_stride_k=max_len)
        # step 0 of a beam search: only the first b rows exist, no history is read
        check(dev, a, logits[:b], words, 0, SEP, b, None, True, b=b, hist_stride_s=beam * max_len, hist_stride_k=max_len)


def test_a_base_that_is_not_16_byte_aligned(dev):
    """ld a multiple of 4 floats but the first row one float past a 16-byte boundary: the scalar path; the floats around stay"""
    from valor_amd import decode, kernels as K
    a = zoo()
    V, ld, R, t = 1000, 1024, 5, 1
    g = torch.Generator().manual_seed(4)
    logits = torch.randn((R, V), generator=g)
    hist = histories(R, V, g)
    store = torch.full((R * ld + 8,), MARK, dtype=torch.float32, device=dev)
    view = store[1:1 + R * ld].view(R, ld)[:, :V]
    view.copy_(logits.to(dev))
    assert view.data_ptr() % 16 == 4
    K.trie_constrain(view, hist.to(dev), t, SEP, a.device(dev))
    assert same_bits(view.cpu(), decode.trie_rows_host(logits, hist, t, a, SEP, R))
    rest = store.clone()
    rest[1:1 + R * ld].view(R, ld)[:, :V] = MARK
    assert (rest == MARK).all()


def test_eager_issue_equals_graph_replay(dev):
    from valor_amd import decode, kernels as K
    a = zoo()
    V, R, t = 30522, 64, 2
    g = torch.Generator().manual_seed(2)
    logits = torch.randn((R, V), generator=g)
    hist = histories(R, V, g)
    hist_dev = hist.to(dev)
    act = torch.ones(R, dtype=torch.bool)
    act[::5] = False
    act_dev = act.to(dev)
    trie = a.device(dev)                                                            # (no host-to-device copy inside the capture)
    eager, eview = buffers(logits, dev, True)
    K.trie_constrain(eview, hist_dev, t, SEP, trie, act_dev)
    torch.cuda.synchronize()
    static, sview = buffers(logits, dev, True)
    fresh = static.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.trie_constrain(sview, hist_dev, t, SEP, trie, act_dev)                    # warm-up on the capture stream
        static.copy_(fresh)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            K.trie_constrain(sview, hist_dev, t, SEP, trie, act_dev)
        static.copy_(fresh)
        graph.replay()
    torch.cuda.synchronize()
    assert same_bits(static.cpu(), eager.cpu())
    assert same_bits(eview.cpu(), decode.trie_rows_host(logits, hist, t, a, SEP, R, act))
