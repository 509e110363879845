"""CPU: the host side of pair alignments (valor_amd/search.py): align_pairs_host against the integer reference of
tests/contrastive_exact.py, credits_host on hand-made rows, the argument checks of valor_fine_align_pairs (they run before any launch,
so a CPU-only host can call them), what explain refuses, and the token layout: inferred, checked, saved and reloaded."""
import ctypes

import pytest
import torch

import contrastive_exact as CE
import search_align_cases as AC


# ------------------------------------------------------------------ 1. the law
@pytest.mark.parametrize("shape", [CE.FUSED_SHAPES[1], CE.FUSED_SHAPES[4], CE.FUSED_SHAPES[7]], ids=lambda s: s.name)
def test_align_pairs_host_is_the_integer_reference_gathered(shape):
    from valor_amd.search import align_pairs_host
    assert AC.census_holds(shape) is None
    texts = [0, 3, shape.NA - 1]
    cand = AC.candidate_rows(3, 9, shape.NB, seed=shape.seed)
    got = align_pairs_host(*AC.exact_inputs(shape, texts), cand, sim=True)
    want = AC.exact_expected(shape, texts, cand)
    for name in AC.OUTPUTS:
        assert CE.first_mismatch(got[name], want[name]) is None, (name, CE.first_mismatch(got[name], want[name]))
    assert got["idx_a"].dtype == torch.uint8 and got["credit_a"].dtype == torch.float32 and got["score"].dtype == torch.float64
    assert align_pairs_host(*AC.exact_inputs(shape, texts), cand)["sim"] is None
    # these inputs are dyadic: either credit array sums to the score exactly
    ok = (cand >= 0) & (cand < shape.NB)
    assert ok.any() and not ok.all()
    assert torch.equal(got["credit_a"].double().sum(-1)[ok], got["score"][ok]) and torch.equal(got["credit_b"].double().sum(-1)[ok], got["score"][ok])
    assert bool((got["score"][ok] != 0).any())


@pytest.mark.parametrize("shape", CE.FUSED_SHAPES, ids=lambda s: s.name)
def test_every_exact_shape_keeps_its_planted_classes_under_an_all_ones_clip_mask(shape):
    case, ref = AC.exact_case(shape)
    CE.check_exactness_conditions(case, ref)
    assert AC.census_holds(shape) is None, AC.census_holds(shape)
    assert bool((CE.case_for(shape).maskB == 0).any()) or shape.Nv == 1          # the cached case itself is untouched


def test_credits_host_on_hand_made_rows():
    from valor_amd.search import credits_host
    # two words on one frame: words 0 and 2 both pick frame 1; frame 1 picks word 2; frame 0 picks word 1
    a2b, idx_a = torch.tensor([0.5, 0.25, 0.75]), torch.tensor([1, 0, 1], dtype=torch.uint8)
    b2a, idx_b = torch.tensor([0.25, 0.75]), torch.tensor([1, 2], dtype=torch.uint8)
    wA, wB = torch.tensor([0.5, 0.25, 0.25]), torch.tensor([0.5, 0.5])
    ca, cb = credits_host(a2b, idx_a, b2a, idx_b, wA, wB)
    termA, termB = [0.125, 0.03125, 0.09375], [0.0625, 0.1875]
    assert cb.tolist() == [termB[0] + termA[1], termB[1] + termA[0] + termA[2]]
    assert ca.tolist() == [termA[0], termA[1] + termB[0], termA[2] + termB[1]]
    assert float(ca.sum()) == float(cb.sum()) == sum(termA) + sum(termB)
    # a zero-weight frame: its term is 0 whatever its maximum (the fused kernel's guard), and it still collects the words that pick it
    ca, cb = credits_host(torch.tensor([0.5]), torch.tensor([0], dtype=torch.uint8), torch.tensor([float("-inf"), 0.25]),
                          torch.tensor([0, 0], dtype=torch.uint8), torch.tensor([1.0]), torch.tensor([0.0, 1.0]))
    assert cb.tolist() == [0.25, 0.125] and ca.tolist() == [0.25 + 0.0 + 0.125]
    # a masked word whose 0 is the maximum: word 1 is masked (x = 0, weight 0), frame 0 sees only negatives and picks it
    a2b, idx_a = torch.tensor([-0.5, 0.0]), torch.tensor([0, 0], dtype=torch.uint8)
    b2a, idx_b = torch.tensor([0.0]), torch.tensor([1], dtype=torch.uint8)
    ca, cb = credits_host(a2b, idx_a, b2a, idx_b, torch.tensor([1.0, 0.0]), torch.tensor([1.0]))
    assert ca.tolist() == [-0.25, 0.0] and cb.tolist() == [-0.25]
    # the additions are fp32, one by one, in ascending order: 1 + 2^-24 + 2^-24 stays 1 (each step rounds to even), 2^-23 would not
    e = 2.0 ** -24
    ca, cb = credits_host(torch.tensor([2.0, 2 * e, 2 * e]), torch.tensor([0, 0, 0], dtype=torch.uint8), torch.tensor([0.0]),
                          torch.tensor([0], dtype=torch.uint8), torch.ones(3), torch.tensor([0.0]))
    assert cb.tolist() == [1.0] and cb.dtype == torch.float32
    # index bytes of 255 (an empty slot) hit nothing, and leading dimensions broadcast
    ca, cb = credits_host(torch.zeros((2, 3, 4)), torch.full((2, 3, 4), 255, dtype=torch.uint8), torch.zeros((2, 3, 5)),
                          torch.full((2, 3, 5), 255, dtype=torch.uint8), torch.ones((2, 1, 4)), torch.ones((2, 3, 5)))
    assert ca.shape == (2, 3, 4) and cb.shape == (2, 3, 5) and not bool(ca.any()) and not bool(cb.any())


# ------------------------------------------------------------------ 2. the entry point's argument checks
def test_align_kernel_validates_before_any_launch():
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    outs = ("score", "a2b", "idx_a", "b2a", "idx_b", "credit_a", "credit_b", "sim")

    def align(**kw):
        a = dict(fa=p, ma=p, wa=p, store=p, ws=p, NS=50, cand=p, ld_cand=8, NA=2, C=7, T=6, Nv=10, D=128, **{n: p for n in outs})
        a.update(kw)
        return so.valor_fine_align_pairs(None, a["fa"], a["ma"], a["wa"], a["store"], a["ws"], a["NS"], a["cand"], a["ld_cand"], a["NA"], a["C"],
                                         a["T"], a["Nv"], a["D"], *[a[n] for n in outs])

    for name in ("fa", "ma", "wa", "store", "ws", "cand"):
        assert align(**{name: None}) == -1, name
    assert align(D=96) == -1 and align(D=0) == -1 and align(D=32) == -1
    assert align(T=0) == -1 and align(T=65) == -1 and align(Nv=0) == -1 and align(Nv=65) == -1
    assert align(ld_cand=6) == -1
    assert align(fa=p + 8) == -1 and align(store=p + 8) == -1 and align(cand=p + 4) == -1 and align(ma=p + 2) == -1
    for name in ("score", "a2b", "b2a", "credit_a", "credit_b", "sim"):
        assert align(**{name: p + 2}) == -1, name
    assert align(NA=-1) == -1 and align(C=-1) == -1 and align(NS=-1) == -1
    # an index array and its value array come together
    assert align(idx_a=None) == -1 and align(a2b=None) == -1 and align(idx_b=None) == -1 and align(b2a=None) == -1
    assert align(NA=0) == 0 and align(C=0) == 0 and align(NA=0, fa=None) == 0


# ------------------------------------------------------------------ 3. the index: refusals and the token layout
def _feats(n=4, tokens=10, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, tokens, 128), generator=g).bfloat16(), torch.softmax(torch.randn((n, tokens), generator=g), -1)


def test_explain_refuses_what_rescore_refuses():
    from valor_amd.search import RetrievalIndex, quantize_rows_host
    feats, w = _feats()
    cand = torch.zeros((2, 3), dtype=torch.int64)
    q = {"feat_t": torch.zeros((2, 6, 128), dtype=torch.bfloat16)}
    coarse = RetrievalIndex("tv", "coarse", False, [torch.zeros((4, 128), dtype=torch.bfloat16)], [None], list(range(4)))
    with pytest.raises(ValueError, match="fine banks"):
        coarse.explain(None, {"feat_t": torch.zeros((2, 128), dtype=torch.bfloat16)}, cand)
    fp32 = RetrievalIndex("tv", "fine", False, [feats.float()], [w], list(range(4)))
    with pytest.raises(ValueError, match="bf16 banks"):
        fp32.explain(None, {"feat_t": torch.zeros((2, 6, 128))}, cand)
    codes, scales = quantize_rows_host(feats)
    plain = RetrievalIndex("tv", "fine", False, [codes], [w], list(range(4)), "fp8", scales=[scales], dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="exact store"):
        plain.explain(None, q, cand)
    for index, queries in ((coarse, {"feat_t": torch.zeros((2, 128), dtype=torch.bfloat16)}), (plain, q)):
        with pytest.raises(ValueError, match="fine banks|exact store"):                 # before anything is encoded or scored
            index.search(None, queries, 2, explain=True)


def test_token_layout_is_inferred_checked_saved_and_reloaded(tmp_path):
    from valor_amd.search import Alignment, AlignmentPart, RetrievalIndex
    feats, w = _feats()
    ids = list(range(4))
    tv = RetrievalIndex("tv", "fine", False, [feats], [w], ids)
    ta = RetrievalIndex("ta", "fine", False, [feats], [w], ids)
    late = RetrievalIndex("tva", "fine", True, [feats[:, :8].contiguous(), feats[:, 8:].contiguous()], [w[:, :8].contiguous(), w[:, 8:].contiguous()], ids)
    assert tv.token_layout == [[("video", 10)]] and ta.token_layout == [[("audio", 10)]]
    assert late.token_layout == [[("video", 8)], [("audio", 2)]]
    fused = RetrievalIndex("tva", "fine", False, [feats], [w], ids)
    assert fused.token_layout is None
    assert RetrievalIndex("tv", "coarse", False, [feats[:, 0].contiguous()], [None], ids).token_layout is None
    given = RetrievalIndex("tva", "fine", False, [feats], [w], ids, token_layout=[[("video", 8), ("audio", 2)]])
    assert given.token_layout == [[("video", 8), ("audio", 2)]]
    via = RetrievalIndex.from_features(feats, w, ids, group="tva", weights_softmaxed=True, token_layout=[("video", 8), ("audio", 2)])
    assert via.token_layout == given.token_layout
    # checked: the counts cover the tokens, the modalities are known, an inferable layout cannot be contradicted
    for bad in ([[("video", 8), ("audio", 3)]], [[("video", 10)], [("audio", 2)]], [[("picture", 10)]], [[("video", 0), ("audio", 10)]], [["video"]]):
        with pytest.raises(ValueError, match="token_layout"):
            RetrievalIndex("tva", "fine", False, [feats], [w], ids, token_layout=bad)
    with pytest.raises(ValueError, match="token_layout"):
        RetrievalIndex("tv", "fine", False, [feats], [w], ids, token_layout=[[("audio", 10)]])
    assert RetrievalIndex("tv", "fine", False, [feats], [w], ids, token_layout=[[("video", 10)]]).token_layout == tv.token_layout
    # add_features checks the counts
    more, mw = _feats(2, 10, seed=2)
    given.add_features([more], [mw], [4, 5], token_layout=[[("video", 8), ("audio", 2)]])
    given.add_features([more], [mw], [6, 7])
    assert len(given) == 8
    with pytest.raises(ValueError, match="token_layout"):
        given.add_features([more], [mw], [8, 9], token_layout=[[("video", 7), ("audio", 3)]])
    short, sw = _feats(2, 9, seed=3)
    with pytest.raises(ValueError, match="tokens per clip"):
        given.add_features([short], [sw], [8, 9])
    assert len(given) == 8
    # saved as an extra key outside the fingerprint, reloaded; an inferred layout needs no key
    assert "token_layout" not in given.fingerprint() and given.fingerprint() == fused.fingerprint()
    given.save(tmp_path / "given.pt")
    blob = torch.load(tmp_path / "given.pt", map_location="cpu", weights_only=True)
    assert blob["token_layout"] == [[["video", 8], ["audio", 2]]] and blob["format"] == "valor_amd.RetrievalIndex/1"
    back = RetrievalIndex.load(tmp_path / "given.pt", "cpu")
    assert back.token_layout == given.token_layout and back.fingerprint() == given.fingerprint() and len(back) == 8
    tv.save(tmp_path / "tv.pt")
    assert "token_layout" not in torch.load(tmp_path / "tv.pt", map_location="cpu", weights_only=True)
    assert RetrievalIndex.load(tmp_path / "tv.pt", "cpu").token_layout == tv.token_layout
    # a file saved without the key loads: the layout is None, and only the per-modality methods refuse
    del blob["token_layout"]
    torch.save(blob, tmp_path / "old.pt")
    old = RetrievalIndex.load(tmp_path / "old.pt", "cpu")
    assert old.token_layout is None and len(old) == 8 and torch.equal(old.feats[0], given.feats[0])
    out = dict(score=torch.zeros((1, 2)), a2b=None, idx_a=None, b2a=None, idx_b=None, credit_a=None, credit_b=torch.zeros((1, 2, 10)), sim=None)
    blind = Alignment(torch.zeros((1, 2), dtype=torch.int64), [AlignmentPart(out, None)])
    for method in (blind.clip_credit_by_modality, blind.best_clip_token):
        with pytest.raises(ValueError, match="token_layout"):
            method()


def test_alignment_methods_on_hand_made_credits():
    from valor_amd.search import Alignment, AlignmentPart
    part = lambda credit, layout: AlignmentPart(dict(score=None, a2b=None, idx_a=None, b2a=None, idx_b=None, credit_a=None, credit_b=credit, sim=None), layout)
    #                       video 0..2        audio 0..1
    fused = torch.tensor([[[0.25, 0.5, 0.5, 0.125, 0.5], [0.0, 0.0, 0.0, 0.0, 0.0], [-1.0, -0.5, -2.0, -0.5, -3.0]]])
    al = Alignment(torch.tensor([[7, -1, 2]]), [part(fused, [("video", 3), ("audio", 2)])])
    by = al.clip_credit_by_modality()
    assert by["video"].tolist() == [[1.25, 0.0, -3.5]] and by["audio"].tolist() == [[0.625, 0.0, -3.5]]
    p, m, j = al.best_clip_token()
    assert (p.tolist(), m.tolist(), j.tolist()) == ([[0, -1, 0]], [[0, -1, 0]], [[1, -1, 1]])          # the lowest index among equals; -1 = empty
    # two parts (late fusion): the credits are compared across the parts, the modality sums added over them
    al = Alignment(torch.tensor([[3]]), [part(torch.tensor([[[0.5, 0.25]]]), [("video", 2)]), part(torch.tensor([[[0.125, 0.5, 0.75]]]), [("audio", 3)])])
    assert [t.tolist() for t in al.best_clip_token()] == [[[1]], [[0]], [[2]]]
    by = al.clip_credit_by_modality()
    assert by["video"].tolist() == [[0.75]] and by["audio"].tolist() == [[1.375]]


def test_search_result_still_iterates_as_three():
    from valor_amd.search import SearchResult
    res = SearchResult(torch.zeros((1, 2)), torch.tensor([[1, -1]]), ["a", "b"])
    ids, scores, indices = res
    assert ids == [["b", None]] and res.alignment is None and len(list(res)) == 3
