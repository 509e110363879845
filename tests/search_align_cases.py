"""Host side shared by tests/test_search_align_cpu.py and tests/test_search_align_gpu.py: the exact cases of tests/contrastive_exact.py
turned into pair-alignment cases (the clip mask set to ones, as valor_fine_align_pairs has it), candidate rows with entries outside the
store, the expected outputs gathered from the integer reference, and random unit-vector inputs on the pattern of
tests/test_search_rescore_gpu.py. Nothing here touches the GPU library at import time."""
from functools import lru_cache

import numpy as np
import torch

import contrastive_exact as CE

OUTPUTS = ("score", "a2b", "idx_a", "b2a", "idx_b", "credit_a", "credit_b", "sim")
ATOL, RTOL = 2e-5, 1e-5          # the project's band for this score path (tests/test_search_rescore_gpu.py)


@lru_cache(maxsize=None)
def exact_case(shape):
    """(case, reference) of a contrastive_exact shape with maskB = ones: a new ExactCase, the cached one stays as it is"""
    base = CE.case_for(shape)
    arrays = {k: v for k, v in base.__dict__.items() if k != "shape"}
    arrays["maskB"] = np.ones_like(base.maskB)
    case = CE.ExactCase(base.shape, **arrays)
    return case, CE.reference(case)


def census_holds(shape):
    """the planted structure survives the all-ones clip mask: None, or what is missing. Every class is asked for where the shape admits
    it at all (contrastive_exact.eligible_classes; a masked slot can now only be a text slot, so masked_is_max needs T >= 2 and shows
    on the B2A axis)."""
    case, ref = exact_case(shape)
    T, Nv = shape.T, shape.Nv
    cen = CE.census(case, ref)
    eligible = CE.eligible_classes(T, Nv)
    missing = [k for k in ("same_lane_tie", "cross_lane_tie", "negative_max", "cross_block_tie") if k in eligible and cen["all"][k] < 1]
    if T >= 2 and cen["B2A"]["masked_is_max"] < 1:
        missing.append("B2A masked_is_max")
    if cen["A2B"]["masked_is_max"] != 0:
        missing.append("A2B masked_is_max must be empty under an all-ones clip mask")
    return missing or None


def candidate_rows(NA, C, NS, seed):
    """int64 [NA, C]: unsorted indices into [0, NS) with -1, NS, 2^40 and a duplicate planted (C >= 7), or one entry per row that is
    in range, -1, NS in turn (shorter rows)"""
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(0, NS, (NA, C), generator=g)
    if C >= 7:
        cand[:, 1], cand[:, 2], cand[:, 3], cand[:, 4] = -1, NS, 1 << 40, cand[:, 0]
        cand[:, 5], cand[:, 6] = NS - 1, 0
    else:
        cand[:, 0] = torch.tensor([NS - 1, -1, NS])[:NA]
    return cand


def exact_inputs(shape, texts):
    """CPU tensors (featA bf16 [len(texts), T, D], maskA, wA, store bf16 [NB, Nv, D], wstore) of the exact case's texts `texts`"""
    case, _ = exact_case(shape)
    texts = list(texts)
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).float()
    return (f32(case.featA[texts]).bfloat16(), f32(case.maskA[texts]), f32(case.wA[texts]), f32(case.featB).bfloat16(), f32(case.wB))


def exact_expected(shape, texts, cand):
    """every output of the kernel for the pairs (texts[a], cand[a, c]), from the integer reference: a dict of fp64 / uint8 tensors. The
    credits follow the stated fp32 sequence on the reference's maxima (credits_host); on these dyadic inputs every step is exact."""
    from valor_amd.search import credits_host
    case, ref = exact_case(shape)
    NB = shape.NB
    texts = torch.tensor(list(texts))
    cand = cand.long()
    ok = (cand >= 0) & (cand < NB)
    safe = torch.where(ok, cand, torch.zeros_like(cand))
    pick = lambda name: torch.from_numpy(np.ascontiguousarray(ref[name]))[texts[:, None], safe]
    live = lambda t, fill: torch.where(ok.view(ok.shape + (1,) * (t.dim() - 2)), t, torch.full_like(t, fill))
    out = dict(score=live(pick("score"), float("-inf")), a2b=live(pick("A2B"), 0.0), b2a=live(pick("B2A"), 0.0), sim=live(pick("x"), 0.0),
               idx_a=live(pick("idxA"), 255), idx_b=live(pick("idxB"), 255))
    wB = live(torch.from_numpy(case.wB)[safe], 0.0)
    out["credit_a"], out["credit_b"] = credits_host(out["a2b"], out["idx_a"], out["b2a"], out["idx_b"], torch.from_numpy(case.wA)[texts][:, None, :], wB)
    return out


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _soft(raw, mask):
    return torch.softmax(raw.masked_fill(mask == 0, float("-inf")), dim=-1)


def random_case(NA, C, T, Nv, D, NS, seed):
    """queries whose first text points AWAY from every clip (all its dot products negative, so the 0 of a masked token wins max_t),
    masks with trailing zeros, non-uniform weights; candidate rows as candidate_rows"""
    g = torch.Generator().manual_seed(seed)
    u = _unit(torch.randn((D,), generator=g))
    store = _unit(_unit(torch.randn((NS, Nv, D), generator=g)) + 0.7 * u).bfloat16()
    fa = _unit(torch.randn((NA, T, D), generator=g))
    fa[0] = _unit(fa[0] - 1.5 * u)
    fa = fa.bfloat16()
    lens = torch.randint(1, T + 1, (NA,), generator=g)
    lens[0] = max(1, T - 2)
    mask = (torch.arange(T)[None] < lens[:, None]).float()
    wa, ws = _soft(torch.randn((NA, T), generator=g), mask), torch.softmax(2 * torch.randn((NS, Nv), generator=g), -1)
    return fa, mask, wa, store, ws, candidate_rows(NA, C, NS, seed + 1)


def check_random_outputs(out, want, wa, ws_pairs, ok):
    """the properties of section 2 on CPU copies `out` of the kernel's outputs (sim included); want: align_pairs_host(..., sim=True) of
    the same inputs; wa [NA, T]; ws_pairs [NA, C, Nv] the clips' weights gathered (anything at empty slots); ok [NA, C] bool. Returns
    the largest |sim - law|. No index is compared with an fp64 arg max."""
    from valor_amd.search import credits_host
    sim, a2b, b2a = out["sim"], out["a2b"], out["b2a"]
    ia, ib = out["idx_a"].long(), out["idx_b"].long()
    err = (sim.double() - want["sim"]).abs()
    assert bool((err <= ATOL + RTOL * want["sim"].abs()).all()), float(err.max())
    # empty slots: -inf, 255, zeros
    assert bool((out["score"][~ok] == float("-inf")).all()) and bool((ia[~ok] == 255).all()) and bool((ib[~ok] == 255).all())
    for name in ("a2b", "b2a", "credit_a", "credit_b", "sim"):
        assert bool((out[name][~ok] == 0).all()), name
    # live pairs: the maximum is the similarity at its index, bit for bit; nothing exceeds it; no earlier slot equals it
    s, A, B, IA, IB = sim[ok], a2b[ok], b2a[ok], ia[ok], ib[ok]                      # [P, T, Nv], [P, T], [P, Nv]
    Tn, Nv = s.shape[1:]
    assert int(IA.max()) < Nv and int(IB.max()) < Tn
    assert torch.equal(s.gather(2, IA[:, :, None])[:, :, 0], A) and torch.equal(s.gather(1, IB[:, None, :])[:, 0, :], B)
    assert bool((s <= A[:, :, None]).all()) and bool((s <= B[:, None, :]).all())
    before_a = torch.arange(Nv)[None, None, :] < IA[:, :, None]
    before_b = torch.arange(Tn)[None, :, None] < IB[:, None, :]
    assert not bool(((s == A[:, :, None]) & before_a).any()) and not bool(((s == B[:, None, :]) & before_b).any())
    # the credits: the stated fp32 sequence on the kernel's own maxima and indices, bit for bit
    ca, cb = credits_host(a2b, out["idx_a"], b2a, out["idx_b"], wa[:, None, :], torch.where(ok[:, :, None], ws_pairs, torch.zeros_like(ws_pairs)))
    assert torch.equal(out["credit_a"], ca) and torch.equal(out["credit_b"], cb)
    return float(err.max())
