"""Pair alignments on the GPU (csrc/search_align.hip) and what stands on them in search.RetrievalIndex: explain, search(explain=True), the
token layout and the per-modality credit.

1. On the exact inputs of tests/contrastive_exact.py (the clip mask set to ones) every output of valor_fine_align_pairs has ONE right
   answer: tolerance zero, guarded buffers, every planted class of ties present. 2. On random unit vectors the similarities are held to
   the fp64 law inside the band of this score path, and everything else to the similarities THE KERNEL wrote: the maxima are elements of
   them at the reported indices, no earlier slot is equal, the credits are the stated fp32 sequence bit for bit. No index is compared
   with an fp64 arg max. 3. Segmented staging and a store beyond 2 GiB. 4. Refusals launch nothing. 5., 6. The index level."""
import pytest
import torch

import contrastive_exact as CE
import search_align_cases as AC

pytestmark = pytest.mark.gpu


def _run_guarded(dev, fa, mask, wa, store, ws, cand, NS=None, ld_cand=None, skip=()):
    """valor_fine_align_pairs into guarded buffers (an output named in `skip` is passed as NULL): ({name: view}, [(buf, view), ...])"""
    from valor_amd import kernels as K, lib
    NA, T, D = fa.shape
    Nv = store.shape[1]
    C = cand.shape[1]
    ld_cand = ld_cand or C
    shapes = dict(score=(NA, C), a2b=(NA, C, T), idx_a=(NA, C, T), b2a=(NA, C, Nv), idx_b=(NA, C, Nv), credit_a=(NA, C, T), credit_b=(NA, C, Nv),
                  sim=(NA, C, T, Nv))
    pairs = {n: CE.guarded(shapes[n], torch.uint8 if n.startswith("idx") else torch.float32, dev) for n in AC.OUTPUTS if n not in skip}
    d = [t.to(dev).contiguous() for t in (fa, mask, wa, store, ws)]
    cand_d = torch.full((NA, ld_cand), 1 << 50, dtype=torch.int64, device=dev)      # only C columns are read
    cand_d[:, :C] = cand.to(dev)
    lib.call("valor_fine_align_pairs", K._stream(), *[t.data_ptr() for t in d], store.shape[0] if NS is None else NS, cand_d.data_ptr(), ld_cand,
             NA, C, T, Nv, D, *[pairs[n][1].data_ptr() if n in pairs else None for n in AC.OUTPUTS])
    torch.cuda.synchronize()
    return {n: v for n, (_, v) in pairs.items()}, list(pairs.values())


def _all_written_and_guards_intact(pairs):
    for buf, view in pairs:
        assert CE.guard_intact(buf, view), "written outside an output"
        v = view.cpu()
        assert not bool((v == CE.PREFILL_U8).any() if v.dtype == torch.uint8 else torch.isnan(v).any()), "an output element was left unwritten"


# ------------------------------------------------------------------ 1. exact, tolerance zero
@pytest.mark.parametrize("shape", CE.FUSED_SHAPES, ids=lambda s: s.name)
def test_every_output_is_the_integer_reference_at_tolerance_zero(dev, shape):
    case, ref = AC.exact_case(shape)
    CE.check_exactness_conditions(case, ref)                              # an inexact case fails as a case
    assert AC.census_holds(shape) is None, AC.census_holds(shape)
    runs = 0
    for NA in (1, 3):
        for C in (1, 7, 33):
            # C = 33 walks every text of the case, the shorter lists a rotating choice of them
            starts = range(0, shape.NA - NA + 1, NA) if C == 33 else [(5 * C + NA) % (shape.NA - NA + 1)]
            for a0 in starts:
                texts = list(range(a0, a0 + NA))
                cand = AC.candidate_rows(NA, C, shape.NB, seed=100 * shape.seed + 10 * C + NA + a0)
                out, pairs = _run_guarded(dev, *AC.exact_inputs(shape, texts), cand, ld_cand=C + 3)
                _all_written_and_guards_intact(pairs)
                want = AC.exact_expected(shape, texts, cand)
                for name in AC.OUTPUTS:
                    bad = CE.first_mismatch(out[name], want[name])
                    assert bad is None, (name, NA, C, a0, bad)
                runs += 1
    assert runs >= 6


def test_null_outputs_leave_the_others_as_they_are(dev):
    """each output may be NULL on its own (an index array goes with its value array): the remaining ones do not change"""
    shape = CE.FUSED_SHAPES[8]
    texts, cand = [0, 3, 4], AC.candidate_rows(3, 7, shape.NB, seed=3)
    full, _ = _run_guarded(dev, *AC.exact_inputs(shape, texts), cand)
    for skip in (("score",), ("a2b", "idx_a"), ("b2a", "idx_b"), ("credit_a",), ("credit_b",), ("sim",), ("score", "a2b", "idx_a", "b2a", "idx_b", "sim"),
                 ("credit_a", "credit_b", "sim")):
        out, pairs = _run_guarded(dev, *AC.exact_inputs(shape, texts), cand, skip=skip)
        _all_written_and_guards_intact(pairs)
        assert set(out) == set(AC.OUTPUTS) - set(skip)
        for name in out:
            assert torch.equal(out[name], full[name]), (skip, name)


# ------------------------------------------------------------------ 2. random unit vectors
NS = 50


def _check_random(dev, NA, C, T, Nv, D, seed, identical):
    from valor_amd.search import align_pairs_host, score_pairs
    fa, mask, wa, store, ws, cand = AC.random_case(NA, C, T, Nv, D, NS, seed)
    out, pairs = _run_guarded(dev, fa, mask, wa, store, ws, cand)
    _all_written_and_guards_intact(pairs)
    want = align_pairs_host(fa, mask, wa, store, ws, cand, sim=True)
    ok = (cand >= 0) & (cand < NS)
    cpu = {n: t.cpu() for n, t in out.items()}
    worst = AC.check_random_outputs(cpu, want, wa, ws[cand.clamp(0, NS - 1)], ok)
    pair = score_pairs(*[t.to(dev).contiguous() for t in (fa, mask, wa, store, ws, cand)]).cpu()
    err = (cpu["score"][ok].double() - pair[ok].double()).abs()
    assert bool((err <= AC.ATOL + AC.RTOL * pair[ok].double().abs()).all()), float(err.max())
    err = (cpu["score"][ok].double() - want["score"][ok]).abs()
    assert bool((err <= AC.ATOL + AC.RTOL * want["score"][ok].abs()).all()), float(err.max())
    identical.append(torch.equal(cpu["score"], pair))
    return worst, want


@pytest.mark.parametrize("T,Nv", [(1, 1), (5, 10), (16, 17), (33, 64), (64, 10), (17, 33)])
def test_random_unit_vectors_against_the_law_and_the_kernels_own_similarities(dev, T, Nv):
    worst, identical, negative_won = 0.0, [], False
    for D in (64, 512):
        for NA, C in ((1, 1), (3, 7), (3, 33)):
            w, want = _check_random(dev, NA, C, T, Nv, D, 1000 * T + 10 * Nv + NA + C + D, identical)
            worst = max(worst, w)
            negative_won = negative_won or bool((want["score"][0][torch.isfinite(want["score"][0])] < 0).any())
    print(f"T {T} Nv {Nv}: largest |sim - fp64 law| {worst:.3g}; score bit-identical to valor_fine_score_pairs: {all(identical)} ({sum(identical)} of {len(identical)})")
    if T > 2:
        assert negative_won, "the case must hold pairs of negative score (real negatives under the 0 of a masked token)"


# ------------------------------------------------------------------ 3. staging and addressing
def test_a_long_query_is_staged_in_segments(dev):
    """a query image above the LDS budget goes through LDS in segments along D, restaged per round of candidates; 33 candidates = three
    workgroups of up to four rounds"""
    identical = []
    worst, _ = _check_random(dev, 2, 33, 64, 10, 1024, 7, identical)
    print(f"T 64 Nv 10 D 1024: largest |sim - fp64 law| {worst:.3g}; score bit-identical to valor_fine_score_pairs: {identical[0]}")


def test_clips_past_two_gib_of_store(dev):
    """a store of 2.16 GB (33 000 clips of 64 tokens x 512): the last clips lie past byte offset 2^31, where a 32-bit offset would wrap.
    Only the rows the candidates name are filled (and known to the host law, which sees them as a store of four)."""
    from valor_amd.search import align_pairs, align_pairs_host
    big, Nv, D, T, NA = 33000, 64, 512, 5, 2
    fa, mask, wa, rows, ws, _ = AC.random_case(NA, 7, T, Nv, D, NS, seed=9)
    rows, ws = rows[:4], ws[:4]
    where = torch.tensor([big - 1, big - 2, 32768, 0])                   # 32768 * 65536 bytes = 2^31 exactly
    store = torch.empty((big, Nv, D), dtype=torch.bfloat16, device=dev)
    wstore = torch.zeros((big, Nv), device=dev)
    store[where.to(dev)], wstore[where.to(dev)] = rows.to(dev), ws.to(dev)
    local = torch.tensor([[0, 1, 2, 3, -1, 4, 1], [3, 2, 1, 0, 0, -1, 4]])        # 4 = outside the store
    ok = (local >= 0) & (local < 4)
    cand = torch.where(ok, where[local.clamp(0, 3)], torch.where(local < 0, local, torch.full_like(local, big)))
    want = align_pairs_host(fa, mask, wa, rows, ws, local, sim=True)
    got = align_pairs(*[t.to(dev).contiguous() for t in (fa, mask, wa)], store, wstore, cand.to(dev), sim=True)
    AC.check_random_outputs({n: t.cpu() for n, t in got.items()}, want, wa, ws[local.clamp(0, 3)], ok)


# ------------------------------------------------------------------ 4. bad arguments
def test_bad_arguments_launch_nothing(dev):
    from valor_amd import kernels as K, lib
    so = lib.load()
    NA, C, T, Nv, D = 2, 7, 6, 10, 128
    fa, mask, wa, store, ws, cand = [t.to(dev).contiguous() for t in AC.random_case(NA, C, T, Nv, D, NS, seed=5)]
    shapes = dict(score=(NA, C), a2b=(NA, C, T), idx_a=(NA, C, T), b2a=(NA, C, Nv), idx_b=(NA, C, Nv), credit_a=(NA, C, T), credit_b=(NA, C, Nv),
                  sim=(NA, C, T, Nv))
    pairs = {n: CE.guarded(shapes[n], torch.uint8 if n.startswith("idx") else torch.float32, dev) for n in AC.OUTPUTS}

    def align(**kw):
        a = dict(fa=fa.data_ptr(), ld_cand=C, T=T, Nv=Nv, D=D, NS=NS, **{n: pairs[n][1].data_ptr() for n in AC.OUTPUTS})
        a.update(kw)
        return so.valor_fine_align_pairs(K._stream(), a["fa"], mask.data_ptr(), wa.data_ptr(), store.data_ptr(), ws.data_ptr(), a["NS"], cand.data_ptr(),
                                         a["ld_cand"], NA, C, a["T"], a["Nv"], a["D"], *[a[n] for n in AC.OUTPUTS])

    untouched = lambda: all(bool((v.cpu() == CE.PREFILL_U8).all() if v.dtype == torch.uint8 else torch.isnan(v.cpu()).all()) for _, v in pairs.values())
    assert align(fa=None) == -1 and align(D=96) == -1 and align(T=65) == -1 and align(Nv=0) == -1 and align(ld_cand=C - 1) == -1 and align(NS=-1) == -1
    assert align(idx_a=None) == -1 and align(b2a=None) == -1 and align(fa=fa.data_ptr() + 8) == -1 and align(sim=pairs["sim"][1].data_ptr() + 2) == -1
    torch.cuda.synchronize()
    assert untouched() and all(CE.guard_intact(b, v) for b, v in pairs.values())
    assert align() == 0
    torch.cuda.synchronize()
    _all_written_and_guards_intact(list(pairs.values()))


# ------------------------------------------------------------------ 5. the index
NB, NV, T, D, NQ, TOPK = 300, 4, 6, 128, 5, 5
PART_NAMES = ("score", "text_max", "text_best", "clip_max", "clip_best", "text_credit", "clip_credit", "sim")


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(21)
    unit = lambda x: torch.nn.functional.normalize(x, dim=-1)
    fb = unit(torch.randn((NB, NV, D), generator=g)).bfloat16()
    fa = unit(torch.randn((NQ, T, D), generator=g)).bfloat16()
    mask = (torch.arange(T)[None] < torch.randint(3, T + 1, (NQ, 1), generator=g)).float()
    wa, wb = torch.randn((NQ, T), generator=g), torch.randn((NB, NV), generator=g)
    subset = torch.stack([torch.randperm(NB, generator=g)[:40] for _ in range(NQ)])
    subset[:, 7], subset[:, 30], subset[:, 12] = subset[:, 3], subset[:, 3], -1     # repeats and a -1
    return dict(fa=fa, fb=fb, mask=mask, wa=wa, wb=wb, subset=subset)


def _queries(c, dev):
    return {"feat_t": c["fa"].to(dev), "mask": c["mask"].to(dev), "weight": c["wa"].to(dev)}


def _index(c, dev, bank_dtype=None, exact=None):
    from valor_amd.search import RetrievalIndex
    return RetrievalIndex.from_features(c["fb"].to(dev), c["wb"].to(dev), [f"c{j}" for j in range(NB)], group="tv", bank_dtype=bank_dtype, exact=exact)


def _same_part(a, b):
    for name in PART_NAMES:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        assert x is None or (x.dtype == y.dtype and torch.equal(x, y)), name
    assert a.layout == b.layout


def test_explain_equals_align_pairs_on_the_bank(dev, case):
    from valor_amd.search import AlignmentPart, align_pairs
    index, q = _index(case, dev), _queries(case, dev)
    cand = case["subset"].to(dev)
    al = index.explain(None, q, cand, sim=True)
    assert torch.equal(al.indices, cand) and len(al.parts) == 1 and al.parts[0].layout == [("video", NV)]
    ft, mask, wq = index._queries(None, q)
    _same_part(al.parts[0], AlignmentPart(align_pairs(ft, mask, wq, index.feats[0], index.weights[0], cand, sim=True), [("video", NV)]))
    part = al.parts[0]
    assert part.text_best.dtype == torch.uint8 and part.sim.shape == (NQ, 40, T, NV) and part.text_credit.shape == (NQ, 40, T)
    assert index.explain(None, q, cand).parts[0].sim is None
    empty = cand < 0
    assert bool((part.score[empty] == float("-inf")).all()) and bool((part.clip_best[empty] == 255).all()) and bool((part.clip_credit[empty] == 0).all())
    # the alignment's score is the pair score of rescore(), inside the band (bit-identity is not promised: DESIGN.md 3.4)
    res = index.rescore(None, q, cand)
    err = (part.score[~empty] - res[~empty]).abs().double()
    assert bool((err <= AC.ATOL + AC.RTOL * res[~empty].abs().double()).all())
    # either credit array sums to the score, to rounding
    for credit in (part.text_credit, part.clip_credit):
        assert float((credit.double().sum(-1)[~empty] - part.score[~empty].double()).abs().max()) <= 1e-5


def test_late_fusion_gives_one_alignment_per_part(dev, case):
    from valor_amd.search import AlignmentPart, RetrievalIndex, align_pairs
    fv, fa = case["fb"][:, :3].contiguous().to(dev), case["fb"][:, 3:].contiguous().to(dev)
    index = RetrievalIndex.from_features([fv, fa], group="tva", late_fusion=True)
    assert index.token_layout == [[("video", 3)], [("audio", 1)]]
    q = {"feat_t": case["fa"].to(dev), "mask": case["mask"].to(dev)}
    cand = case["subset"].to(dev)
    al = index.explain(None, q, cand)
    ft, mask, wq = index._queries(None, q)
    for p, (store, layout) in enumerate(((fv, [("video", 3)]), (fa, [("audio", 1)]))):
        _same_part(al.parts[p], AlignmentPart(align_pairs(ft, mask, wq, store, index.weights[p], cand), layout))
    ok = cand >= 0
    total = al.parts[0].score + al.parts[1].score
    res = index.rescore(None, q, cand)
    assert bool(((total[ok] - res[ok]).abs() <= 2 * (AC.ATOL + AC.RTOL * float(res[ok].abs().max()))).all())
    by = al.clip_credit_by_modality()
    assert torch.equal(by["video"], al.parts[0].clip_credit.sum(-1)) and torch.equal(by["audio"], al.parts[1].clip_credit.sum(-1))
    part, modality, token = al.best_clip_token()
    assert bool((part[~ok] == -1).all()) and bool(((part[ok] == 0) | (part[ok] == 1)).all()) and bool((modality[ok] == 0).all())
    assert bool((token[ok][part[ok] == 1] == 0).all()) and bool((token[ok] < 3).all())


def test_fp8_banks_with_either_store_give_the_bf16_alignment(dev, case):
    q = _queries(case, dev)
    cand = case["subset"].to(dev)
    want = _index(case, dev).explain(None, q, cand, sim=True)
    for store in ("device", "host"):
        got = _index(case, dev, "fp8", store).explain(None, q, cand, sim=True)
        assert torch.equal(got.indices, want.indices)
        _same_part(got.parts[0], want.parts[0])


def test_search_with_explain_returns_the_same_search_on_all_three_paths(dev, case):
    q = _queries(case, dev)
    cand = case["subset"].to(dev)
    plain, two_stage, host = _index(case, dev), _index(case, dev, "fp8", "device"), _index(case, dev, "fp8", "host")
    for index, kw in ((plain, {}), (plain, dict(within=cand)), (two_stage, dict(shortlist=20)), (host, dict(shortlist=20)), (two_stage, dict(within=cand))):
        ref = index.search(None, q, TOPK, **kw)
        res = index.search(None, q, TOPK, explain=True, **kw)
        assert ref.alignment is None and torch.equal(res.scores, ref.scores) and torch.equal(res.indices, ref.indices) and res.ids == ref.ids
        ids, scores, indices = res                                        # still a 3-tuple
        assert indices is res.indices
        assert torch.equal(res.alignment.indices, res.indices)
        _same_part(res.alignment.parts[0], index.explain(None, q, res.indices).parts[0])
        assert res.alignment.parts[0].sim is None
        with_sim = index.search(None, q, TOPK, explain=True, sim=True, **kw)
        assert torch.equal(with_sim.indices, ref.indices) and with_sim.alignment.parts[0].sim.shape == (NQ, TOPK, T, NV)
    with pytest.raises(ValueError, match="exact store"):
        _index(case, dev, "fp8").search(None, q, TOPK, explain=True)


def test_k_larger_than_the_bank_leaves_empty_slots(dev, case):
    from valor_amd.search import RetrievalIndex
    index = RetrievalIndex.from_features(case["fb"][:3].to(dev), case["wb"][:3].to(dev), group="tv")
    res = index.search(None, _queries(case, dev), TOPK, explain=True, sim=True)
    assert bool((res.indices[:, 3:] == -1).all()) and bool((res.indices[:, :3] >= 0).all())
    part = res.alignment.parts[0]
    assert bool((part.text_best[:, 3:] == 255).all()) and bool((part.clip_best[:, 3:] == 255).all()) and bool((part.score[:, 3:] == float("-inf")).all())
    for t in (part.text_max, part.clip_max, part.text_credit, part.clip_credit, part.sim):
        assert bool((t[:, 3:] == 0).all())
    assert bool((part.text_best[:, :3] < NV).all()) and bool((part.clip_best[:, :3] < T).all())
    best = res.alignment.best_clip_token()
    assert all(bool((b[:, 3:] == -1).all()) and bool((b[:, :3] >= 0).all()) for b in best)


# ------------------------------------------------------------------ 6. modality credit
def test_a_query_made_of_one_audio_token_credits_the_audio(dev):
    """a fused 'tva' bank on exact inputs (ternary features, weights in multiples of 2^-6), 8 video + 2 audio tokens per clip; the video
    tokens live on the first half of the feature dimensions and the audio tokens on the second, and the query is ONE token: the first
    audio token of clip 4. The picture then has similarity 0 with it, every number is a short dyadic, and the credits have one right
    answer, computed here from the integer dot products."""
    import numpy as np
    from valor_amd.search import RetrievalIndex
    rng = np.random.default_rng(41)
    clips, Dm, target, token = 9, 64, 4, 8
    fb = np.zeros((clips, 10, Dm), dtype=np.float32)
    fb[:, :8, :32] = rng.integers(-1, 2, size=(clips, 8, 32))
    fb[:, 8:, 32:] = rng.integers(-1, 2, size=(clips, 2, 32))
    fb = torch.from_numpy(fb)
    wb = torch.from_numpy(rng.integers(1, 65, size=(clips, 10)).astype(np.float32) / 64.0)     # softmaxed as far as the index knows
    index = RetrievalIndex.from_features(fb.bfloat16().to(dev), wb.to(dev), group="tva", weights_softmaxed=True, token_layout=[("video", 8), ("audio", 2)])
    assert index.token_layout == [[("video", 8), ("audio", 2)]]
    query = fb[target, token]
    dots = fb[target] @ query                                             # the ten integer similarities of the pair
    assert bool((dots[:8] == 0).all()) and float(dots[token]) >= 8 and float(dots[token]) > float(dots[9])
    # one query token, mask 1, weight softmax(one value) = 1: a2b = dots[token] at `token`; b2a = dots, every clip token's best (only) word
    want_b = 0.5 * (wb[target] * dots)
    want_b[token] += 0.5 * dots[token]
    want_score = 0.5 * (float(dots[token]) + float((wb[target].double() * dots.double()).sum()))
    q = {"feat_t": query.bfloat16().view(1, 1, Dm).to(dev)}
    al = index.explain(None, q, torch.tensor([[target, -1]], device=dev))
    part = al.parts[0]
    assert part.text_best[0, 0].tolist() == [token] and part.text_max[0, 0].tolist() == [float(dots[token])]
    assert part.clip_best[0, 0].tolist() == [0] * 10 and torch.equal(part.clip_max[0, 0].cpu(), dots)
    assert torch.equal(part.clip_credit[0, 0].cpu(), want_b) and float(part.score[0, 0]) == want_score
    assert part.text_credit[0, 0].tolist() == [want_score]
    by = al.clip_credit_by_modality()
    assert float(by["video"][0, 0]) == 0.0 and float(by["audio"][0, 0]) == want_score > 0      # the sound carries the whole match
    assert float(by["audio"][0, 1]) == 0.0 and float(by["video"][0, 1]) == 0.0                 # the empty slot
    p, m, j = al.best_clip_token()
    assert (p[0].tolist(), m[0].tolist(), j[0].tolist()) == ([0, -1], [1, -1], [token - 8, -1])
    res = index.search(None, q, 2, explain=True)
    assert target in res.indices[0].tolist()
    slot = res.indices[0].tolist().index(target)
    assert float(res.alignment.clip_credit_by_modality()["audio"][0, slot]) == want_score
