"""Closed answer sets without a GPU: the AnswerSet trie (shared prefixes, duplicates, per-sample roots, ascending children,
from_bert_rows, every ValueError, index_of), the host law of valor_trie_constrain (decode.trie_rows_host) on hand-made rows, the
argument validation of valor_trie_constrain before any launch, and the argument errors of the generate_* / validate_qa interface."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import decode, synth                    # noqa: E402
from valor_amd.model.valor import VALOR                 # noqa: E402

SEP, CLS = 102, 101
INF = float("inf")


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def children(a, node):
    lo, hi = int(a.child_ptr[node]), int(a.child_ptr[node + 1])
    return a.child_tok[lo:hi].tolist(), a.child_node[lo:hi].tolist()


def walk(a, root, toks):
    node = root
    for w in toks:
        tk, nd = children(a, node)
        if w not in tk:
            return -1
        node = nd[tk.index(w)]
    return node


# ------------------------------------------------------------------------------------------------ the trie
def test_trie_shares_prefixes_and_orders_children():
    cands = [[7, 8, 9], [7, 8], [7, 5], [300, 4], [20], [7, 8, 9]]                 # 5 is a duplicate of 0
    a = decode.AnswerSet(cands)
    assert not a.per_sample and a.n_roots == 1 and a.root.tolist() == [0] and a.max_len == 3 and a.counts == [6]
    # nodes: root, 7, 7-8, 7-8-9, 7-5, 300, 300-4, 20
    assert a.n_nodes == 8 and a.child_tok.numel() == 7
    assert a.child_ptr.dtype == a.child_tok.dtype == a.child_node.dtype == a.root.dtype == torch.int32 and a.terminal.dtype == torch.uint8
    assert a.child_ptr.numel() == a.n_nodes + 1 and int(a.child_ptr[0]) == 0 and int(a.child_ptr[-1]) == 7
    for n in range(a.n_nodes):
        tk, nd = children(a, n)
        assert tk == sorted(tk) and len(set(tk)) == len(tk) and all(0 < c < a.n_nodes for c in nd)
    assert children(a, 0)[0] == [7, 20, 300]
    n78 = walk(a, 0, [7, 8])
    assert children(a, walk(a, 0, [7]))[0] == [5, 8] and children(a, n78)[0] == [9]
    assert bool(a.terminal[n78]) and bool(a.terminal[walk(a, 0, [7, 8, 9])]) and not bool(a.terminal[walk(a, 0, [7])])
    assert not bool(a.terminal[0]) and int(a.terminal.sum()) == 5
    assert a.index_of(torch.tensor([[7, 8, 9, SEP], [7, 8, SEP, 9], [20, SEP, SEP, SEP]])).tolist() == [0, 1, 4]


def test_per_sample_roots_and_duplicates():
    a = decode.AnswerSet([[[7, 8], [9]], [[7, 8], [7, 8], [7]], [[11]]], per_sample=True)
    assert a.per_sample and a.n_roots == 3 and len(set(a.root.tolist())) == 3 and a.counts == [2, 3, 1]
    r0, r1, r2 = a.root.tolist()
    assert children(a, r0)[0] == [7, 9] and children(a, r1)[0] == [7] and children(a, r2)[0] == [11]
    assert walk(a, r0, [7, 8]) != walk(a, r1, [7, 8])                             # the samples share no node
    assert bool(a.terminal[walk(a, r1, [7])]) and not bool(a.terminal[walk(a, r0, [7])])
    # index_of: row r reads sample r % n_roots; the lowest index among duplicates; -1 outside the set
    seqs = torch.tensor([[7, 8, SEP], [7, 8, SEP], [11, SEP, 0], [9, SEP, 0], [7, SEP, 5], [7, SEP, 0]])
    assert a.index_of(seqs).tolist() == [0, 0, 0, 1, 2, -1]
    assert a.index_of(torch.tensor([[SEP, 7, 8], [8, SEP, 0], [12, 3, 4]])).tolist() == [-1, -1, -1]
    assert a.index_of(torch.tensor([[7, 8]])).tolist() == [0]                       # no [SEP]: the whole row
    assert a.index_of(seqs).dtype == torch.int64
    # re-rooting for several rows per sample
    e = a.for_rows(6)
    assert e.root.tolist() == [r0, r0, r1, r1, r2, r2] and e.counts == [2, 2, 3, 3, 1, 1]
    assert a.for_rows(4, [1, 2, 1]).root.tolist() == [r0, r1, r1, r2] and a.for_rows(3) is a
    with pytest.raises(ValueError, match="does not describe"):
        a.for_rows(5)
    shared = decode.AnswerSet([[7]])
    assert shared.for_rows(17) is shared


def test_from_bert_rows():
    rows = torch.tensor([[CLS, 7, 8, SEP, 0, 0], [CLS, 9, SEP, 0, 0, 0], [CLS, 7, 8, 9, 10, SEP], [CLS, 11, SEP, 0, 0, 0]])
    a = decode.AnswerSet.from_bert_rows(rows)
    assert a.candidates == [[[7, 8], [9], [7, 8, 9, 10], [11]]] and a.n_roots == 1 and a.max_len == 4
    p = decode.AnswerSet.from_bert_rows(rows, per_sample_counts=[1, 3])
    assert p.per_sample and p.candidates == [[[7, 8]], [[9], [7, 8, 9, 10], [11]]]
    with pytest.raises(ValueError, match="per_sample_counts"):
        decode.AnswerSet.from_bert_rows(rows, per_sample_counts=[1, 2])
    with pytest.raises(ValueError, match="CLS"):
        decode.AnswerSet.from_bert_rows(torch.tensor([[7, 8, SEP]]))
    with pytest.raises(ValueError, match="CLS"):
        decode.AnswerSet.from_bert_rows(torch.tensor([[CLS, 7, 8, 0]]))
    with pytest.raises(ValueError, match="empty"):
        decode.AnswerSet.from_bert_rows(torch.tensor([[CLS, SEP, 0]]))


def test_answer_set_value_errors():
    with pytest.raises(ValueError, match="empty"):
        decode.AnswerSet([[7], []])
    with pytest.raises(ValueError, match="empty"):
        decode.AnswerSet([])
    with pytest.raises(ValueError, match="sample 1 is empty"):
        decode.AnswerSet([[[7]], []], per_sample=True)
    for bad in (0, -1, SEP, 1.5):
        with pytest.raises(ValueError, match="holds id"):
            decode.AnswerSet([[7, bad]])
    with pytest.raises(ValueError, match="holds id"):
        decode.AnswerSet([[7, 40]], vocab=40)
    decode.AnswerSet([[7, 39]], vocab=40)
    a = decode.AnswerSet([[7, 1199], [1200]])
    with pytest.raises(ValueError, match="vocabulary"):
        a.check_vocab(1200)
    a.check_vocab(1201)


# ------------------------------------------------------------------------------------------------ the host law
def floor_bits():
    return torch.tensor(decode.TRIE_FLOOR, dtype=torch.float32)


def test_floor_is_the_fp32_nearest_to_minus_1e30():
    from valor_amd import lib
    assert decode.TRIE_FLOOR == lib.TRIE_FLOOR == float(torch.tensor(-1e30, dtype=torch.float32))
    assert floor_bits().view(torch.int32).item() & 0xFFFFFFFF == 0xF149F2CA
    header = open(os.path.join(ROOT, "include", "valor_hip.h")).read()
    assert "#define VALOR_TRIE_FLOOR (-1e30f)" in header
    # a floored column has no mass beside any ordinary logit
    assert float(torch.exp(floor_bits() - torch.tensor(-1e4))) == 0.0


def allowed_of(out, logits):
    """per row: the columns whose bits survived (the test's logits hold no floor value)"""
    keep = out.view(torch.int32) == logits.view(torch.int32)
    assert ((out == decode.TRIE_FLOOR) | keep).all()
    return [set(torch.nonzero(k).view(-1).tolist()) for k in keep]


def test_trie_rows_host_on_hand_made_rows():
    V, eos = 40, 2
    a = decode.AnswerSet([[7, 8], [7, 8, 9], [7, 5], [30]])                        # 7-8 is terminal AND has a child
    g = torch.Generator().manual_seed(3)
    logits = torch.randn((6, V), generator=g)
    logits[0, 3], logits[1, 4], logits[2, 5] = -0.0, -INF, 1e-41               # bits that must survive where the column is allowed / inactive
    logits[:, 39] = float("nan")
    hist = torch.tensor([[7, 8, 0], [7, 5, 0], [7, 8, 9], [30, 0, 0], [9, 9, 9], [7, 8, 0]])
    keep0 = logits.clone()
    # t = 0: the root's children; [SEP] is closed (the root is no end)
    out = decode.trie_rows_host(logits, None, 0, a, eos, 6)
    assert same_bits(logits, keep0)                                                 # the input is not modified
    assert out.dtype == torch.float32 and all(s == {7, 30} for s in allowed_of(out, logits))
    assert same_bits(out[:, 7], logits[:, 7]) and (out[:, 39] == decode.TRIE_FLOOR).all()
    # t = 1
    got = allowed_of(decode.trie_rows_host(logits, hist, 1, a, eos, 6), logits)
    assert got == [{5, 8}, {5, 8}, {5, 8}, {eos}, {eos}, {5, 8}]                    # a leaf allows only [SEP]; 9 is off the trie: only [SEP]
    # t = 2: terminal with children, leaf, off-trie after a valid first token
    got = allowed_of(decode.trie_rows_host(logits, hist, 2, a, eos, 6), logits)
    assert got == [{9, eos}, {eos}, {9, eos}, {eos}, {eos}, {9, eos}]
    # t = 3: [7 8 0] left the trie at the id 0
    got = allowed_of(decode.trie_rows_host(logits, hist, 3, a, eos, 6), logits)
    assert got == [{eos}, {eos}, {eos}, {eos}, {eos}, {eos}]
    # inactive rows keep every bit, NaN and -inf included
    active = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.uint8)
    out = decode.trie_rows_host(logits, hist, 2, a, eos, 6, active)
    for r in (1, 3, 5):
        assert same_bits(out[r], logits[r])
    assert allowed_of(out[[0, 2, 4]], logits[[0, 2, 4]]) == [{9, eos}, {9, eos}, {eos}]
    # untouched columns keep their bits: -0.0 in an allowed column
    z = logits.clone()
    z[0, 9] = -0.0
    o = decode.trie_rows_host(z, hist, 2, a, eos, 6)
    assert o[0, 9].view(torch.int32).item() == torch.tensor(-0.0).view(torch.int32).item()
    # history ids that are [SEP], >= V or negative have no edge
    h2 = torch.tensor([[eos, 7], [V + 5, 7], [-3, 7], [7, eos], [7, V], [7, 8]])
    got = allowed_of(decode.trie_rows_host(logits, h2, 2, a, eos, 6), logits)
    assert got == [{eos}] * 5 + [{9, eos}]


def test_trie_rows_host_per_sample_roots_and_token_range():
    V, eos = 20, 2
    a = decode.AnswerSet([[[5], [6, 7]], [[8]], [[6, 9]]], per_sample=True)
    logits = torch.arange(6 * V, dtype=torch.float32).view(6, V)
    got = allowed_of(decode.trie_rows_host(logits, None, 0, a, eos, 3), logits)     # rows 3..5 are the second beam: sample r % 3
    assert got == [{5, 6}, {8}, {6}] * 2
    hist = torch.tensor([[6], [8], [6], [5], [6], [9]])
    got = allowed_of(decode.trie_rows_host(logits, hist, 1, a, eos, 3), logits)
    assert got == [{7}, {eos}, {9}, {eos}, {eos}, {eos}]
    with pytest.raises(ValueError, match="roots"):
        decode.trie_rows_host(logits, None, 0, a, eos, 6)
    # a candidate token >= V names no column (the set was built for a larger vocabulary)
    big = decode.AnswerSet([[5], [25]])
    assert allowed_of(decode.trie_rows_host(logits, None, 0, big, eos, 6), logits) == [{5}] * 6


# ------------------------------------------------------------------------------------------------ the C entry, without a GPU
def test_library_exports_the_symbol_and_the_binding_knows_it():
    from valor_amd import kernels as K, lib
    so = lib.load()
    assert hasattr(so, "valor_trie_constrain") and len(lib.SIGNATURES["valor_trie_constrain"]) == 20
    assert callable(K.trie_constrain)
    if not torch.cuda.is_available():
        a = decode.AnswerSet([[7]])
        with pytest.raises(lib.ValorHipError):                     # no CPU fallback
            K.trie_constrain(torch.zeros(2, 8), None, 0, 3, a.device("cpu"))


def test_trie_constrain_validates_arguments_without_gpu():
    from valor_amd import lib
    so = lib.load()
    f = (ctypes.c_float * 64)()
    i64 = (ctypes.c_int64 * 64)()
    ptr = (ctypes.c_int32 * 4)(0, 2, 2, 2)
    tok = (ctypes.c_int32 * 2)(5, 6)
    nod = (ctypes.c_int32 * 2)(1, 2)
    term = (ctypes.c_uint8 * 3)(0, 1, 1)
    root = (ctypes.c_int32 * 4)(0, 0, 0, 0)
    u8 = (ctypes.c_uint8 * 4)()

    def call(R=4, V=16, ld=16, t=3, eos=3, logits=f, hist=i64, ss=8, sk=0, b=4, cp=ptr, ct=tok, cn=nod, tm=term, rt=root, nn=3, ne=2, nr=1,
             act=u8):
        return so.valor_trie_constrain(None, logits, ld, R, V, hist, ss, sk, b, t, eos, cp, ct, cn, tm, rt, nn, ne, nr, act)
    assert call(R=0) == 0 and call(R=0, logits=None, hist=None, cp=None) == 0       # no rows: no-op, nothing is launched
    assert call(logits=None) == -1 and call(hist=None) == -1
    assert call(cp=None) == -1 and call(ct=None) == -1 and call(cn=None) == -1 and call(tm=None) == -1 and call(rt=None) == -1
    assert call(R=-1) == -1 and call(V=0) == -1 and call(ld=15) == -1 and call(t=-1) == -1 and call(t=513) == -1
    assert call(eos=16) == -1 and call(eos=-1) == -1
    assert call(b=0) == -1 and call(ss=-1) == -1 and call(sk=-8) == -1
    assert call(nr=0) == -1 and call(nr=2) == -1 and call(nr=3) == -1 and call(nr=5) == -1
    assert call(nn=0) == -1 and call(nn=-1) == -1 and call(ne=-1) == -1
    with pytest.raises(lib.ValorHipError, match="valor_trie_constrain failed with code -1"):
        lib.call("valor_trie_constrain", None, ctypes.addressof(f), 16, 4, 16, None, 8, 0, 4, 3, 3, ctypes.addressof(ptr), ctypes.addressof(tok),
                 ctypes.addressof(nod), ctypes.addressof(term), ctypes.addressof(root), 3, 2, 1, None)          # null hist with t > 0


# ------------------------------------------------------------------------------------------------ the interface
def test_generate_and_validate_argument_errors_and_signatures():
    import inspect
    from valor_amd import evaluate
    m = VALOR({"max_generation_len": 6}, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu")
    qa = lambda **kw: decode.generate_qa(m, {}, ["tv"], torch.zeros((1, 4), dtype=torch.long), **kw)
    cap = lambda **kw: decode.generate_cap(m, {}, ["tv"], **kw)
    for gen in (cap, qa):
        for rule in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_length=1), dict(suppress_tokens=(5,))):
            with pytest.raises(ValueError, match="candidates"):
                gen(candidates=[[7, 8]], **rule)
        with pytest.raises(ValueError, match="longest answer"):
            gen(candidates=[[7], [7, 8, 9, 10, 11, 12]])                         # 6 tokens and [SEP] do not fit in 6 - 1
        with pytest.raises(ValueError, match="vocabulary"):
            gen(candidates=[[7, 1200]])
        with pytest.raises(ValueError, match="holds id"):
            gen(candidates=[[7, 0]])
        with pytest.raises(ValueError, match="empty"):
            gen(candidates=[[7], []])
    for fn in (decode.generate_cap, decode.generate_qa, decode.decode_greedy, decode.decode_beam, decode.decode_sample,
               decode._decode_groups):
        assert inspect.signature(fn).parameters["candidates"].default is None
    p = inspect.signature(decode.score_candidates).parameters
    assert list(p)[:4] == ["model", "batch", "groups", "candidates"] and p["prompt_cpu"].default is None and p["max_rows"].default == 512
    p = inspect.signature(evaluate.validate_qa).parameters
    assert p["candidates"].default is None and p["multiple_choice"].default is False
    for fn in (VALOR.forward, VALOR.forward_cap, VALOR.forward_qa):
        assert inspect.signature(fn).parameters["candidates"].default is None
    with pytest.raises(ValueError, match="candidates"):
        m.forward({}, "ret%tv", compute_loss=False, candidates=decode.AnswerSet([[7]]))
    with pytest.raises(ValueError, match="candidates"):
        m.forward_cap({}, "cap%tv", compute_loss=True, candidates=decode.AnswerSet([[7]]))
    with pytest.raises(ValueError, match="multiple_choice"):
        evaluate.validate_qa(m, [], "qa%tv", candidates=[[7]], multiple_choice=True)
    with pytest.raises(ValueError, match="same number of choices"):
        evaluate._choice_sets({"choice_tokens": {"bert_tokens": torch.tensor([[CLS, 7, SEP]] * 5)}}, 2)
    with pytest.raises(ValueError, match="differ"):
        evaluate._choice_sets({"choice_tokens": {"bert_tokens": torch.tensor([[CLS, 7, SEP]] * 4)}, "choice_nums": [1, 3]}, 2)
    with pytest.raises(ValueError, match="integer"):
        evaluate._answer_indices({"answers": ["yes", "no"]})
    assert evaluate._answer_indices({"txt_tokens": torch.tensor([2, 0])}) == [2, 0]
    cs = evaluate._choice_sets({"choice_tokens": {"bert_tokens": torch.tensor([[CLS, 7, SEP], [CLS, 8, SEP], [CLS, 9, SEP], [CLS, 7, SEP]])}}, 2)
    assert cs.per_sample and cs.candidates == [[[7], [8]], [[9], [7]]]
