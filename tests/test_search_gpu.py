"""Retrieval search on the GPU: valor_topk_rows (csrc/search.hip) against its host statement topk_host, exactly; RetrievalIndex.search
against topk_host of the index's own chunked scores, exactly, and against the CPU oracle inside a band; the bank built by a model.

The band: delta = 2e-5 + 1e-5 * |s|, the tolerance tests/test_evaluate_gpu.py grants the device's fine score path against
Oracle.compute_fine_matrix. With s_k the oracle's k-th best score of a query, every returned clip must have an oracle score >= s_k - delta,
every clip whose oracle score is > s_k + delta must be returned, returned scores lie within delta of the oracle's at their indices, and
the returned list is ordered (scores non-increasing, equal scores by ascending index). No query is excluded."""
import dataclasses
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
ATOL, RTOL = 2e-5, 1e-5


def _same(got, want):
    gv, gi = got[0].cpu(), got[1].cpu()
    wv, wi = want
    assert torch.equal(gi, wi), (gi, wi)
    assert torch.equal(torch.isnan(gv), torch.isnan(wv)) and torch.equal(torch.nan_to_num(gv, nan=0.0), torch.nan_to_num(wv, nan=0.0))


def _matrix(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((R, C), generator=g) * 8).round() / 8          # ties


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("C", [1, 7, 64, 257, 4099])
def test_kernel_equals_topk_host(dev, R, C):
    """every k in one case (a launch is microseconds): k > C pads with -inf / -1; C = 4099 spans two column segments"""
    from valor_amd.search import topk_host, topk_rows
    s = _matrix(R, C, 10 * R + C)
    d = s.to(dev)
    for k in (1, 3, 10, 64, 256):
        _same(topk_rows(d, k), topk_host(s, k))


@pytest.mark.parametrize("C,k", [(50000, 256), (50000, 10), (1500, 100)])
def test_kernel_many_segments_and_refills(dev, C, k):
    """one row of 50000 columns: a dozen segments; ascending values refill the candidate buffer at every step (the k-th best rises
    all the time), descending ones never after the first"""
    from valor_amd.search import topk_host, topk_rows
    ramp = torch.arange(C, dtype=torch.float32)[None]
    s = torch.cat((ramp, -ramp, _matrix(1, C, 5), (ramp / 7).floor()), 0)
    _same(topk_rows(s.to(dev), k), topk_host(s, k))


def test_kernel_padded_buffer_and_unaligned_view(dev):
    """ld = C + 3 rounded up to a multiple of 4 with +inf in the tail: 16-byte loads with a masked tail; a view that starts one float
    into the buffer: 4-byte loads"""
    from valor_amd.search import topk_host, topk_rows
    for C in (7, 257, 4099):
        s = _matrix(5, C, C)
        ld = (C + 3 + 3) // 4 * 4
        buf = torch.full((5, ld), float("inf"), device=dev)
        buf[:, :C] = s.to(dev)
        assert buf.data_ptr() % 16 == 0 and buf.stride(0) % 4 == 0
        _same(topk_rows(buf[:, :C], 10), topk_host(s, 10))
        flat = torch.full((5 * ld + 1,), float("inf"), device=dev)
        view = flat[1:].view(5, ld)[:, :C]
        view.copy_(s.to(dev))
        assert view.data_ptr() % 16 == 4
        _same(topk_rows(view, 10), topk_host(s, 10))


def test_kernel_ties_nan_and_inf(dev):
    from valor_amd.search import topk_host, topk_rows
    val, idx = topk_rows(torch.full((3, 1000), 0.25, device=dev), 64)
    assert torch.equal(idx.cpu(), torch.arange(64)[None].expand(3, 64)) and bool((val == 0.25).all())
    g = torch.Generator().manual_seed(0)
    s = _matrix(5, 4099, 1)
    s[torch.rand(s.shape, generator=g) < 0.2] = float("nan")
    s[torch.rand(s.shape, generator=g) < 0.05] = float("-inf")
    s[3] = float("nan")                                                # a row of NaNs: indices 0 .. k-1
    s[4, 5:] = float("nan")                                            # fewer numbers than k
    s[4, :5] = torch.tensor([-0.0, 0.0, float("-inf"), 1.0, 0.0])
    for k in (10, 256):
        val, idx = topk_rows(s.to(dev), k)
        assert int(idx.min()) >= 0 and int(idx.max()) < 4099           # every index is a candidate's
        _same((val, idx), topk_host(s, k))
        assert idx[3].tolist() == list(range(k)) and idx[4, :5].tolist() == [3, 0, 1, 4, 2]
    val, idx = topk_rows(s[:, :6].contiguous().to(dev), 10)            # k > C: -1 behind the NaNs, nothing else out of range
    assert int(idx.min()) == -1 and int(idx.max()) < 6 and bool((idx[:, 6:] == -1).all()) and bool((idx[:, :6] >= 0).all())


def test_kernel_merges_chunks_with_large_bases(dev):
    from valor_amd.search import topk_host, topk_rows
    s = _matrix(5, 4099, 2)
    d = s.to(dev)
    for k in (10, 256):
        for base in (0, 2 ** 33):
            want = topk_host(s, k, base=base)
            _same(topk_rows(d, k, col_base=base), want)
            state = (torch.full((5, k), float("-inf"), device=dev), torch.full((5, k), -1, dtype=torch.int64, device=dev))
            c0 = 0
            for n in (100, 1, 3998):                                   # merge = 1 onto the empty state first
                topk_rows(d[:, c0:c0 + n], k, col_base=base + c0, state=state)
                c0 += n
            _same(state, want)
            state = (torch.full((5, k), float("-inf"), device=dev), torch.full((5, k), -1, dtype=torch.int64, device=dev))
            c0 = 4099
            for n in (3998, 1, 100):                                   # the chunks in another order: the same result
                c0 -= n
                topk_rows(d[:, c0:c0 + n], k, col_base=base + c0, state=state)
            _same(state, want)
    empty = (torch.full((2, 7), float("-inf"), device=dev), torch.full((2, 7), -1, dtype=torch.int64, device=dev))
    topk_rows(torch.zeros((2, 0), device=dev), 7, state=empty)
    assert bool((empty[1] == -1).all()) and bool(torch.isinf(empty[0]).all())


# ------------------------------------------------------------------ 2. - 4. the index on given features
NB, NV, T, D, NQ, TOPK = 700, 10, 32, 128, 9, 10


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


@pytest.fixture(scope="module")
def fine_case():
    """bf16-rounded unit features, text masks of random length, raw token weights, and the oracle's fp32 scores (computed once)"""
    import valor_oracle as VO
    g = torch.Generator().manual_seed(11)
    fb = _unit(torch.randn((NB, NV, D), generator=g)).bfloat16()
    fa = _unit(torch.randn((NQ, T, D), generator=g)).bfloat16()
    mask = (torch.arange(T)[None] < torch.randint(3, T + 1, (NQ, 1), generator=g)).long()
    wa, wb = torch.randn((NQ, T), generator=g), torch.randn((NB, NV), generator=g)
    want = VO.Oracle.compute_fine_matrix(fa.float(), fb.float(), mask, torch.ones((NB, NV), dtype=torch.long), wa, wb)
    return dict(fa=fa, fb=fb, mask=mask, wa=wa, wb=wb, want=want)


def _fine_index(case, dev):
    from valor_amd.search import RetrievalIndex
    index = RetrievalIndex.from_features(case["fb"].to(dev), case["wb"].to(dev), [f"c{j}" for j in range(NB)], group="tv")
    q = {"feat_t": case["fa"].to(dev), "mask": case["mask"].to(dev).float(), "weight": case["wa"].to(dev)}
    return index, q


@pytest.mark.parametrize("chunk", [64, 257, 700])
def test_index_search_equals_topk_of_its_scores(dev, fine_case, chunk):
    from valor_amd.search import topk_host
    index, q = _fine_index(fine_case, dev)
    res = index.search(None, q, TOPK, chunk=chunk)
    full = index.scores(None, q, chunk=chunk)
    assert full.shape == (NQ, NB) and res.scores.is_cuda and res.indices.dtype == torch.int64
    want = topk_host(full.cpu(), TOPK)
    _same((res.scores, res.indices), want)
    assert res.ids == [[f"c{j}" for j in row] for row in want[1].tolist()]
    ids, scores, indices = res                                          # unpacks as (ids, scores, indices)
    assert ids is res.ids and scores is res.scores and indices is res.indices


def _check_against(want, scores, indices, k):
    """the membership rule of the module docstring; `want` [NQ, NB] reference scores. Prints the measured figures first."""
    scores, indices = scores.cpu(), indices.cpu()
    delta = ATOL + RTOL * want.abs()
    at = want.gather(1, indices)
    dev_err = (scores - at).abs()
    print(f"largest |returned score - reference| {float(dev_err.max()):.3g} (band {float((ATOL + RTOL * at.abs()).min()):.3g} .. "
          f"{float((ATOL + RTOL * at.abs()).max()):.3g})")
    s_k = torch.sort(want, dim=1, descending=True)[0][:, k - 1:k]
    d_k = ATOL + RTOL * s_k.abs()
    assert bool((dev_err <= ATOL + RTOL * at.abs()).all())
    assert bool((at >= s_k - d_k).all())                                 # nothing returned that is clearly worse than the k-th
    must = want > s_k + d_k                                              # clearly better than the k-th: must be there
    got = torch.zeros_like(must)
    got.scatter_(1, indices, True)
    assert bool((got | ~must).all())
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
    tie = scores[:, 1:] == scores[:, :-1]
    assert bool((indices[:, 1:] > indices[:, :-1])[tie].all())
    assert all(len(set(row)) == k for row in indices.tolist())


def test_index_against_the_oracle(dev, fine_case):
    """valor_oracle.Oracle.compute_fine_matrix in fp32 on the bf16-rounded features, band 2e-5 + 1e-5 |s| as specified (the fused bf16 kernel sums
    products of bf16 values in fp32, as the oracle does); the largest deviation is printed before anything is asserted."""
    index, q = _fine_index(fine_case, dev)
    full = index.scores(None, q)
    print(f"largest |device score - oracle| over the matrix {float((full.cpu() - fine_case['want']).abs().max()):.3g}")
    for chunk in (None, 257):
        res = index.search(None, q, TOPK, chunk=chunk)
        _check_against(fine_case["want"], res.scores, res.indices, TOPK)


def test_fp32_bank_takes_the_gemm_path(dev, fine_case):
    """parity mode: fp32 features go through the fp32 GEMM + valor_fine_scores"""
    from valor_amd.search import RetrievalIndex, topk_host
    index = RetrievalIndex.from_features(fine_case["fb"].float().to(dev), fine_case["wb"].to(dev), group="tv")
    q = {"feat_t": fine_case["fa"].float().to(dev), "mask": fine_case["mask"].to(dev).float(), "weight": fine_case["wa"].to(dev)}
    res = index.search(None, q, TOPK, chunk=257)
    _same((res.scores, res.indices), topk_host(index.scores(None, q, chunk=257).cpu(), TOPK))
    _check_against(fine_case["want"], res.scores, res.indices, TOPK)


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_coarse_and_late_fusion_banks(dev, late, dtype):
    """pooled vectors: the scores are K.gemm's (the sum of two under late fusion); search equals topk_host of them for every chunk plan"""
    from valor_amd import kernels as K
    from valor_amd.search import RetrievalIndex, topk_host
    g = torch.Generator().manual_seed(5)
    banks = [_unit(torch.randn((NB, D), generator=g)).to(dtype).to(dev) for _ in range(2 if late else 1)]
    ft = _unit(torch.randn((NQ, D), generator=g)).to(dtype).to(dev)
    index = RetrievalIndex.from_features(banks, group="tva", contra_type="coarse", late_fusion=late)
    want_full = sum(K.gemm(ft, b, out_dtype=torch.float32) for b in banks)
    band = ATOL + RTOL * want_full.abs()
    for chunk in (64, 257, 700):
        full = index.scores(None, {"feat_t": ft}, chunk=chunk)
        assert bool(((full - want_full).abs() <= band).all())
        res = index.search(None, {"feat_t": ft}, TOPK, chunk=chunk)
        _same((res.scores, res.indices), topk_host(full.cpu(), TOPK))
    assert torch.equal(index.scores(None, {"feat_t": ft}, chunk=700), want_full)
    ref = sum(ft.float().cpu() @ b.float().cpu().t() for b in banks)
    res = index.search(None, {"feat_t": ft}, TOPK)
    _check_against(ref, res.scores, res.indices, TOPK)


def test_fine_late_fusion_bank(dev, fine_case):
    """late fusion of a fine model: a video and an audio bank, unit token weights on both sides, the two scores added"""
    import valor_oracle as VO
    from valor_amd.search import RetrievalIndex, topk_host
    fv, fa = fine_case["fb"][:, :6].contiguous(), fine_case["fb"][:, 6:].contiguous()
    index = RetrievalIndex.from_features([fv.to(dev), fa.to(dev)], group="tva", late_fusion=True)
    q = {"feat_t": fine_case["fa"].to(dev), "mask": fine_case["mask"].to(dev).float()}
    ones = lambda f: torch.ones(f.shape[:2])
    cfm = VO.Oracle.compute_fine_matrix
    qa, m = fine_case["fa"].float(), fine_case["mask"]
    want = cfm(qa, fv.float(), m, ones(fv).long(), ones(qa), ones(fv)) + cfm(qa, fa.float(), m, ones(fa).long(), ones(qa), ones(fa))
    res = index.search(None, q, TOPK, chunk=257)
    _same((res.scores, res.indices), topk_host(index.scores(None, q, chunk=257).cpu(), TOPK))
    _check_against(want, res.scores, res.indices, TOPK)


# ------------------------------------------------------------------ 5. end to end
def _batches(spec, seed0, n_batches, clips=4, q=False):
    from valor_amd import synth
    out = []
    for i in range(n_batches):
        b = synth.make_batch(spec, batch=clips, frames=2, audio_slices=1, txt_len=32, seed=seed0 + i, bf16_exact=q)
        b["ids"] = [f"v{clips * i + j}" for j in range(clips)]
        out.append(b)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_index_built_by_a_model(dev, tmp_path, dtype):
    from valor_amd import evaluate as E, synth
    from valor_amd.model.valor import VALOR
    from valor_amd.search import RetrievalIndex
    q = dtype == torch.bfloat16
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05, bf16_exact=q)
    batches = _batches(spec, 70, 4, q=q)
    model = VALOR({"dropout": 0.0}, spec=spec, dtype=dtype, device=dev)
    model.load_state_dict(sd, strict=True)
    model.eval()
    index = RetrievalIndex.build(model, batches[:3], "tva")
    assert len(index) == 12 and index.ids == [f"v{j}" for j in range(12)] and index.dtype == dtype
    # the twelve captions in one query batch; the reference scores from the features of the full 'ret%tva' pass, run as validate_ret runs
    # it: under torch.no_grad. (With autograd on, ops.linear keeps the training step's GEMM kernels; without it, few-row products whose
    # contraction length gemm_skinny.hip covers -- here the ViT patch embedding, 128 rows x K = 768 -- take the weight-streaming kernel,
    # which sums in another order: in bf16 the features then differ in their last bit and the scores by several 1e-5. The index encodes
    # under no_grad, so that is the pass it is held to.)
    with torch.no_grad():
        evs = [model(b, task="ret%tva", compute_loss=False) for b in batches[:3]]
        ft, fv, fa = (torch.cat([e[k] for e in evs], 0).contiguous() for k in ("feat_t", "feat_v", "feat_a"))
        tok = torch.cat([e["txt_tokens"].to(dev) for e in evs], 0)
        fva = torch.cat((fv, fa), dim=1)
        wva = torch.cat((E._fine_weights(model, "video", fv), E._fine_weights(model, "audio", fa)), dim=1)
        want = E.fine_score_matrix(ft, fva, (tok != 0).float(), torch.ones(fva.shape[:2], device=dev), E._fine_weights(model, "text", ft), wva).cpu()
    queries = {"clip_tokens": torch.cat([b["txt_tokens"]["clip_tokens"] for b in batches[:3]], 0),
               "bert_tokens": torch.cat([b["txt_tokens"]["bert_tokens"] for b in batches[:3]], 0)}
    res = index.search(model, queries, 5)
    assert res.scores.shape == (12, 5) and all(i in index.ids for row in res.ids for i in row)
    _check_against(want, res.scores, res.indices, 5)
    one = index.search(model, batches[1], 5)                            # a batch with 'txt_tokens' works as the query too
    _check_against(want[4:8], one.scores, one.indices, 5)
    index.save(tmp_path / "bank.pt")
    back = RetrievalIndex.load(tmp_path / "bank.pt", dev)
    again = back.search(model, queries, 5)
    assert torch.equal(again.scores, res.scores) and torch.equal(again.indices, res.indices) and again.ids == res.ids
    index.add(model, batches[3])                                        # a fourth batch: earlier indices keep their meaning
    assert len(index) == 16 and index.ids[:12] == back.ids and index.ids[12:] == [f"v{j}" for j in range(12, 16)]
    full16, full12 = index.scores(model, queries), back.scores(model, queries)
    assert bool(((full16[:, :12] - full12).abs() <= ATOL + RTOL * full12.abs()).all())
    from valor_amd.search import topk_host
    _same(tuple(index.search(model, queries, 5))[1:], topk_host(full16.cpu(), 5))
    from types import SimpleNamespace
    with pytest.raises(ValueError):                                     # a model with another contrastive head
        index.search(SimpleNamespace(spec=dataclasses.replace(spec, contra_type="coarse")), queries, 5)


@pytest.mark.parametrize("contra,late", [("coarse", False), ("coarse", True), ("fine", True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_model_built_coarse_and_late_fusion_banks(dev, dtype, contra, late):
    """the other branches of encode_gallery ('tva'): va_fusion of the pooled vectors, the two banks of late fusion (coarse and fine), held
    to the scores validate_ret forms from the features of the full 'ret%tva' pass (evaluate.py: the 'tva' group), in the band above"""
    from valor_amd import evaluate as E, kernels as K, ops, synth
    from valor_amd.model.valor import VALOR
    from valor_amd.search import RetrievalIndex
    q = dtype == torch.bfloat16
    spec = dataclasses.replace(synth.tiny_spec(), contra_type=contra, late_fusion=late)
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05, bf16_exact=q)
    batches = _batches(spec, 70, 3, q=q)
    model = VALOR({"dropout": 0.0}, spec=spec, dtype=dtype, device=dev)
    model.load_state_dict(sd, strict=True)
    model.eval()
    index = RetrievalIndex.build(model, batches, "tva")
    assert len(index) == 12 and len(index.feats) == (2 if late else 1) and index.contra_type == contra
    with torch.no_grad():                                               # as validate_ret runs the model
        evs = [model(b, task="ret%tva", compute_loss=False) for b in batches]
        ft, fv, fa = (torch.cat([e[k] for e in evs], 0).contiguous() for k in ("feat_t", "feat_v", "feat_a"))
        if contra == "coarse":
            sim = lambda a, b: K.gemm(a, b, out_dtype=torch.float32)
            if late:
                want = sim(ft, fv) + sim(ft, fa)
            else:
                want = sim(ft, ops.l2_normalize(ops.linear(torch.cat((fv, fa), dim=-1), model.P["va_fusion.weight"], model.P["va_fusion.bias"])))
        else:
            mt = (torch.cat([e["txt_tokens"].to(dev) for e in evs], 0) != 0).float()
            ones = lambda f: torch.ones(f.shape[:2], device=dev)
            want = E.fine_score_matrix(ft, fv, mt, ones(fv), ones(ft), ones(fv)) + E.fine_score_matrix(ft, fa, mt, ones(fa), ones(ft), ones(fa))
    want = want.cpu()
    queries = {"clip_tokens": torch.cat([b["txt_tokens"]["clip_tokens"] for b in batches], 0),
               "bert_tokens": torch.cat([b["txt_tokens"]["bert_tokens"] for b in batches], 0)}
    full = index.scores(model, queries).cpu()
    print(f"largest |index score - reference| over the matrix {float((full - want).abs().max()):.3g}")
    assert bool(((full - want).abs() <= ATOL + RTOL * want.abs()).all())
    res = index.search(model, queries, 5)
    _check_against(want, res.scores, res.indices, 5)
