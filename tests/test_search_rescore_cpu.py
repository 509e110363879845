"""CPU: the host side of pair scores, the subset search and the two-stage search (valor_amd/search.py): pair_scores_host against the
all-pairs law, the plan of search(within=) against an independent ordering, format 3 of the index file beside formats 1 and 2, the
refusals, and the argument checks of valor_fine_score_pairs (they run before any launch, so a CPU-only host can call them)."""
import ctypes

import pytest
import torch


# ------------------------------------------------------------------ 1. the law
def test_pair_scores_host_is_the_all_pairs_law_gathered():
    """features that ARE e4m3 values (exact in bf16) with unit scales: fp8_scores_host on the codes is then the all-pairs bf16 law, no
    dequantisation error in between; pair_scores_host must equal it at the candidate positions and be -inf outside [0, NS)"""
    from valor_amd.search import fp8_scores_host, pair_scores_host
    g = torch.Generator().manual_seed(3)
    NA, NS, T, Nv, D = 3, 11, 5, 7, 64
    codes = lambda *shape: torch.randint(0, 0x7f, shape, generator=g, dtype=torch.uint8) | (torch.randint(0, 2, shape, generator=g, dtype=torch.uint8) << 7)
    ca, cb = codes(NA, T, D), codes(NS, Nv, D)
    fa, fb = ca.view(torch.float8_e4m3fn).float().bfloat16(), cb.view(torch.float8_e4m3fn).float().bfloat16()
    assert torch.equal(fa.float(), ca.view(torch.float8_e4m3fn).float())
    maskA = (torch.arange(T)[None] < torch.tensor([5, 3, 1])[:, None]).float()
    wA = torch.softmax(torch.randn((NA, T), generator=g).masked_fill(maskA == 0, float("-inf")), -1)
    wB = torch.softmax(torch.randn((NS, Nv), generator=g), -1)
    full = fp8_scores_host(ca, torch.ones((NA, T)), cb, torch.ones((NS, Nv)), maskA, torch.ones((NS, Nv)), wA, wB)
    cand = torch.tensor([[4, 4, 0, -1, 10, NS, 1 << 40, 7], [10, 9, 8, 7, 6, 5, 4, 3], [-1, -5, NS + 3, 2, 2, 0, 1, 0]])
    got = pair_scores_host(fa, maskA, wA, fb, wB, cand)
    ok = (cand >= 0) & (cand < NS)
    assert got.dtype == torch.float64 and got.shape == cand.shape
    assert bool((got[~ok] == float("-inf")).all()) and bool(torch.isfinite(got[ok]).all())
    want = full.gather(1, cand.clamp(0, NS - 1))
    assert float((got - want)[ok].abs().max()) <= 1e-9 * float(want[ok].abs().max())
    assert float(got[0, 0]) == float(got[0, 1])                          # a duplicate is scored like any other


# ------------------------------------------------------------------ 2. the plan of search(within=)
def test_within_plan_on_a_hand_made_matrix_with_ties():
    from valor_amd.search import topk_host, within_finish, within_host, within_prepare
    #           clip 0    1    2    3    4    5    6    7
    score = torch.tensor([[0.5, 0.9, 0.5, 0.9, 0.1, 0.9, 0.5, 0.2],
                          [0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3],
                          [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]])
    cand = torch.tensor([[6, 5, 3, 5, -1, 2, 0, 3],                      # unsorted, 5 and 3 twice, a -1
                         [7, 7, 1, 9, 4, -1, 1, 2],                      # 9 is outside the bank of 8
                         [-1, -1, -1, -1, 3, -1, -1, -1]])               # one real candidate
    srt = within_prepare(cand, 8)
    assert srt.tolist() == [[-1, 0, 2, 3, -1, 5, -1, 6], [-1, 1, -1, 2, 4, 7, -1, -1], [-1, -1, -1, -1, -1, -1, -1, 3]]
    val, idx = within_host(score, cand, 4)
    # score descending, then bank index ascending; missing slots -inf / -1
    assert idx.tolist() == [[3, 5, 0, 2], [1, 2, 4, 7], [3, -1, -1, -1]]
    inf = float("-inf")
    assert torch.equal(val, torch.where(idx >= 0, score.gather(1, idx.clamp(min=0)), torch.full(idx.shape, inf))) and val[2, 0] == score[2, 3]
    # against topk_host on the matrix itself, the clips outside each list taken out
    for k in (1, 3, 8):
        val, idx = within_host(score, cand, k)
        for r in range(3):
            members = sorted({int(c) for c in cand[r] if 0 <= int(c) < 8})
            sub_v, sub_i = topk_host(score[r:r + 1, members], k)
            want_i = [members[j] if j >= 0 else -1 for j in sub_i[0].tolist()]
            assert idx[r].tolist() == want_i and val[r].tolist() == sub_v[0].tolist(), (k, r)
    # the two halves the device path shares with the plan
    pair = torch.where(srt >= 0, score.gather(1, srt.clamp(min=0)), torch.full(srt.shape, inf))
    v2, i2 = within_finish(*topk_host(pair, 4), srt)
    assert i2.tolist() == [[3, 5, 0, 2], [1, 2, 4, 7], [3, -1, -1, -1]] and v2[2].tolist()[1:] == [inf] * 3


# ------------------------------------------------------------------ 3. the index file and the refusals
def _cpu_index(bank_dtype=None, exact=None, late=False):
    from valor_amd.search import RetrievalIndex, quantize_rows_host
    g = torch.Generator().manual_seed(1)
    parts = 2 if late else 1
    feats = [torch.randn((6, 10, 128), generator=g).bfloat16() for _ in range(parts)]
    weights = [torch.softmax(torch.randn((6, 10), generator=g), dim=-1) for _ in range(parts)]
    ids = [f"c{j}" for j in range(6)]
    group = "tva" if late else "tv"
    if bank_dtype is None:
        return RetrievalIndex(group, "fine", late, feats, weights, ids, exact=exact), feats
    codes, scales = zip(*[quantize_rows_host(f) for f in feats])
    return RetrievalIndex(group, "fine", late, list(codes), weights, ids, "fp8", scales=list(scales), dtype=torch.bfloat16, exact=exact,
                          exact_feats=feats if exact else None), feats


@pytest.mark.parametrize("exact", ["device", "host"])
@pytest.mark.parametrize("late", [False, True])
def test_format_3_round_trips(tmp_path, exact, late):
    from valor_amd.search import RetrievalIndex
    index, feats = _cpu_index("fp8", exact, late)
    assert index.exact == exact and index.fingerprint()["exact"] == exact and index.fingerprint()["bank_dtype"] == "fp8_e4m3"
    assert all(torch.equal(e, f) and e.dtype == torch.bfloat16 for e, f in zip(index.exact_feats, feats))
    codes_bytes = len(feats) * (6 * 10 * 128 + 2 * 6 * 10 * 4)
    assert index.bank_bytes() == codes_bytes + (len(feats) * 6 * 10 * 128 * 2 if exact == "device" else 0)
    index.save(tmp_path / "bank3.pt")
    blob = torch.load(tmp_path / "bank3.pt", map_location="cpu", weights_only=True)
    assert blob["format"] == "valor_amd.RetrievalIndex/3"
    assert sorted(blob) == ["codes", "exact_feats", "fingerprint", "format", "ids", "scales", "weights"]
    back = RetrievalIndex.load(tmp_path / "bank3.pt", "cpu")
    assert back.exact == exact and back.bank_dtype == "fp8" and back.ids == index.ids and back.fingerprint() == index.fingerprint()
    for a, b in zip(back.feats + back.scales + back.weights + back.exact_feats, index.feats + index.scales + index.weights + index.exact_feats):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # both stores grow with the codes
    assert index._exact[0].data.shape[0] == 6 and len(index._exact) == len(feats)


def test_formats_1_and_2_are_written_and_load_as_before(tmp_path):
    from valor_amd.search import RetrievalIndex
    for bank_dtype, tag, keys in ((None, "/1", ["feats", "fingerprint", "format", "ids", "weights"]),
                                  ("fp8", "/2", ["codes", "fingerprint", "format", "ids", "scales", "weights"])):
        index, _ = _cpu_index(bank_dtype)
        assert index.exact is None and index.exact_feats is None and "exact" not in index.fingerprint()
        path = tmp_path / f"bank{tag[1]}.pt"
        index.save(path)
        blob = torch.load(path, map_location="cpu", weights_only=True)
        assert blob["format"] == "valor_amd.RetrievalIndex" + tag and sorted(blob) == keys
        back = RetrievalIndex.load(path, "cpu")
        assert back.exact is None and back.bank_dtype == bank_dtype and back.fingerprint() == index.fingerprint() and back.ids == index.ids
        for a, b in zip(back.feats + back.weights, index.feats + index.weights):
            assert torch.equal(a, b)


def test_what_the_exact_store_and_the_shortlist_refuse():
    from valor_amd.search import RetrievalIndex
    with pytest.raises(ValueError, match="only an fp8 bank"):
        _cpu_index(None, "device")
    feats = torch.zeros((4, 10, 128), dtype=torch.bfloat16)
    w = torch.full((4, 10), 0.1)
    with pytest.raises(ValueError, match="only an fp8 bank"):
        RetrievalIndex.from_features(feats, w, group="tv", weights_softmaxed=True, exact="host")
    with pytest.raises(ValueError, match="exact"):
        _cpu_index("fp8", "disk")
    with pytest.raises(ValueError, match="bf16 features"):              # codes without the features they were made from
        RetrievalIndex("tv", "fine", False, [torch.zeros((4, 10, 128), dtype=torch.uint8)], [w], list(range(4)), "fp8",
                       scales=[torch.ones((4, 10))], dtype=torch.bfloat16, exact="device")
    with pytest.raises(ValueError, match="bf16 features"):              # an fp32 store: fp32 pair scores are not covered
        RetrievalIndex("tv", "fine", False, [torch.zeros((4, 10, 128), dtype=torch.uint8)], [w], list(range(4)), "fp8",
                       scales=[torch.ones((4, 10))], dtype=torch.float32, exact="device", exact_feats=[feats.float()])
    q = {"feat_t": torch.zeros((2, 6, 128), dtype=torch.bfloat16)}
    index, _ = _cpu_index("fp8", "device")
    assert index.default_shortlist(5) == 20 and index.default_shortlist(100) == 256
    for k, shortlist in ((5, 4), (5, 257), (5, -1), (200, 100)):
        with pytest.raises(ValueError, match="shortlist"):
            index.search(None, q, k, shortlist=shortlist)
    with pytest.raises(ValueError, match="no shortlist"):
        index.search(None, q, 5, within=torch.zeros((2, 3), dtype=torch.int64), shortlist=20)
    plain, _ = _cpu_index("fp8")
    with pytest.raises(ValueError, match="exact store"):
        plain.search(None, q, 5, shortlist=20)
    cand = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="exact store"):                # no fallback to the fp8 scores
        plain.rescore(None, q, cand)
    with pytest.raises(ValueError, match="exact store"):
        plain.search(None, q, 2, within=cand)
    coarse = RetrievalIndex("tv", "coarse", False, [torch.zeros((4, 128), dtype=torch.bfloat16)], [None], list(range(4)))
    with pytest.raises(ValueError, match="fine banks"):
        coarse.rescore(None, {"feat_t": torch.zeros((2, 128), dtype=torch.bfloat16)}, cand)
    fp32 = RetrievalIndex("tv", "fine", False, [feats.float()], [w], list(range(4)))
    with pytest.raises(ValueError, match="bf16 banks"):
        fp32.rescore(None, {"feat_t": torch.zeros((2, 6, 128))}, cand)


# ------------------------------------------------------------------ 4. the entry point's argument checks
def test_pair_kernel_validates_before_any_launch():
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def score(**kw):
        a = dict(fa=p, ma=p, wa=p, store=p, ws=p, NS=50, cand=p, ld_cand=8, out=p, ld_out=8, NA=2, C=7, T=6, Nv=10, D=128)
        a.update(kw)
        return so.valor_fine_score_pairs(None, a["fa"], a["ma"], a["wa"], a["store"], a["ws"], a["NS"], a["cand"], a["ld_cand"], a["out"], a["ld_out"],
                                         a["NA"], a["C"], a["T"], a["Nv"], a["D"])

    for name in ("fa", "ma", "wa", "store", "ws", "cand", "out"):
        assert score(**{name: None}) == -1, name
    assert score(D=96) == -1 and score(D=0) == -1 and score(D=32) == -1
    assert score(T=0) == -1 and score(T=65) == -1 and score(Nv=0) == -1 and score(Nv=65) == -1
    assert score(ld_cand=6) == -1 and score(ld_out=6) == -1
    assert score(fa=p + 8) == -1 and score(store=p + 8) == -1 and score(cand=p + 4) == -1 and score(out=p + 2) == -1
    assert score(NA=-1) == -1 and score(C=-1) == -1 and score(NS=-1) == -1
    assert score(NA=0) == 0 and score(C=0) == 0 and score(NA=0, fa=None) == 0
