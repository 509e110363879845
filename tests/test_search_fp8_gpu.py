"""The fp8 clip bank on the GPU (csrc/search_fp8.hip, search.RetrievalIndex with bank_dtype="fp8").

valor_fp8_quantize_rows is held to quantize_rows_host bit for bit. valor_fine_fused_fwd_fp8 is held to fp8_scores_host (fp64) on the same
codes and scales inside a derived bound per (text, clip) pair:
    D * 2^-23 * max_{t,v}( scaleA scaleB sum_d |codeA codeB| )  +  8 * 2^-24 * |score|
Products of two e4m3 values are exact in fp32, so the first term covers D fp32 additions in any order with unit roundoff 2^-23 (the
MFMA's internal rounding is not documented as round-to-nearest); the second covers the scale multiplies and the weighted token sums.
At D = 512 on unit-norm rows this is about 6e-5, a hundred times below the quantisation error: a wrong operand, scale or slot cannot
hide in it. The index is then held to its own scores (exactly) and to the same host law."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _bound(ca, sa, cb, sb, want):
    """the per-pair tolerance of the module docstring, in fp64 on the CPU"""
    de = lambda c: c.cpu().view(torch.float8_e4m3fn).float().double().abs()
    D = ca.shape[-1]
    mag = torch.einsum("atd,bvd->abtv", de(ca), de(cb)) * sa.cpu().double()[:, None, :, None] * sb.cpu().double()[None, :, None, :]
    return D * 2.0 ** -23 * mag.amax(dim=(2, 3)) + 8 * 2.0 ** -24 * want.abs()


def _soft(raw, mask):
    return torch.softmax(raw.masked_fill(mask == 0, float("-inf")), dim=-1)


# ------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantiser_equals_the_host_law_bit_for_bit(dev, dtype):
    from valor_amd.search import quantize_rows, quantize_rows_host
    g = torch.Generator().manual_seed(7)
    for rows in (1, 5, 257):
        for cols in (16, 128, 512):
            # rows of very different magnitude; a zero row and a tiny row where there is room
            x = torch.randn((rows, cols), generator=g) * torch.exp(4 * torch.randn((rows, 1), generator=g))
            if rows > 2:
                x[1] = 0.0
                x[2] *= 2.0 ** -70
            x = x.to(dtype)
            want_c, want_s = quantize_rows_host(x)
            got_c, got_s = quantize_rows(x.to(dev))
            assert got_c.dtype == torch.uint8 and got_s.dtype == torch.float32
            assert torch.equal(got_c.cpu(), want_c), (rows, cols, int((got_c.cpu() != want_c).sum()))
            assert torch.equal(got_s.cpu(), want_s), (rows, cols)
    wide = (torch.randn((5, 160), generator=g) * 3).to(dtype).to(dev)   # ld = 160 > cols = 128: a column slice of a wider matrix
    view = wide[:, :128]
    assert not view.is_contiguous()
    got_c, got_s = quantize_rows(view)
    want_c, want_s = quantize_rows_host(view.cpu())
    assert got_c.is_contiguous() and torch.equal(got_c.cpu(), want_c) and torch.equal(got_s.cpu(), want_s)
    three = torch.randn((3, 4, 32), generator=g).to(dtype)              # leading dimensions are kept
    got_c, got_s = quantize_rows(three.to(dev))
    assert got_c.shape == (3, 4, 32) and got_s.shape == (3, 4) and torch.equal(got_c.cpu(), quantize_rows_host(three)[0])


def test_quantiser_on_the_hand_made_rows(dev):
    """the rows of tests/test_search_fp8_cpu.py, padded with zeros to 16 columns: subnormal outputs, ties, the sign of zero, the clamp"""
    from test_search_fp8_cpu import HAND_ROWS
    from valor_amd.search import quantize_rows
    x = torch.zeros((len(HAND_ROWS), 16))
    for i, (row, _, _) in enumerate(HAND_ROWS):
        x[i, :len(row)] = torch.tensor(row)
    codes, scales = quantize_rows(x.to(dev))
    for i, (row, want_codes, want_scale) in enumerate(HAND_ROWS):
        got = codes[i].cpu().tolist()
        assert got[:len(row)] == want_codes and not any(got[len(row):]), (row, [hex(c) for c in got])
        assert scales[i].item() == want_scale, (row, scales[i].item().hex())


# ------------------------------------------------------------------ 2. the score kernel
def _score_case(NA, NB, T, Nv, D, seed):
    from valor_amd.search import quantize_rows_host
    g = torch.Generator().manual_seed(seed)
    ca, sa = quantize_rows_host(_unit(torch.randn((NA, T, D), generator=g)))
    cb, sb = quantize_rows_host(_unit(torch.randn((NB, Nv, D), generator=g)))
    lens = torch.randint(1, T + 1, (NA,), generator=g)
    lens[NA // 2] = 1                                                   # one text with a single live token
    maskA = (torch.arange(T)[None] < lens[:, None]).float()
    maskB = torch.ones((NB, Nv))
    wA, wB = _soft(torch.randn((NA, T), generator=g), maskA), _soft(torch.randn((NB, Nv), generator=g), maskB)
    return ca, sa, cb, sb, maskA, maskB, wA, wB


@pytest.mark.parametrize("NA,NB,T,Nv,D", [(1, 1, 1, 1, 128), (3, 5, 7, 10, 128), (9, 17, 32, 10, 512), (5, 9, 33, 17, 256), (2, 3, 64, 64, 128),
                                          (70, 130, 12, 10, 128)])
def test_score_kernel_against_the_host_law(dev, NA, NB, T, Nv, D):
    from valor_amd import kernels as K, lib
    from valor_amd.search import fp8_scores_host
    case = _score_case(NA, NB, T, Nv, D, seed=NA * 1000 + NB)
    want = fp8_scores_host(*case)
    d = [t.to(dev).contiguous() for t in case]
    out = torch.full((NA, NB), float("nan"), device=dev)
    lib.call("valor_fine_fused_fwd_fp8", K._stream(), *[t.data_ptr() for t in d], out.data_ptr(), NA, NB, T, Nv, D)
    err = (out.cpu().double() - want).abs()
    bound = _bound(case[0], case[1], case[2], case[3], want)
    print(f"largest |kernel - host law| {float(err.max()):.3g}; bound {float(bound.min()):.3g} .. {float(bound.max()):.3g}; "
          f"largest ratio {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ 3. - 5. the index on given features
NB, NV, T, D, NQ, TOPK = 1000, 10, 12, 128, 9, 20


@pytest.fixture(scope="module")
def fine_case():
    """bf16 unit features, text masks of random length, raw token weights; the host law's scores on the host-quantised rows (once)"""
    from valor_amd.search import fp8_scores_host, quantize_rows_host
    g = torch.Generator().manual_seed(11)
    fb = _unit(torch.randn((NB, NV, D), generator=g)).bfloat16()
    fa = _unit(torch.randn((NQ, T, D), generator=g)).bfloat16()
    mask = (torch.arange(T)[None] < torch.randint(3, T + 1, (NQ, 1), generator=g)).float()
    wa, wb = torch.randn((NQ, T), generator=g), torch.randn((NB, NV), generator=g)
    ca, sa = quantize_rows_host(fa)
    cb, sb = quantize_rows_host(fb)
    ones = torch.ones((NB, NV))
    want = fp8_scores_host(ca, sa, cb, sb, mask, ones, _soft(wa, mask), _soft(wb, ones))
    return dict(fa=fa, fb=fb, mask=mask, wa=wa, wb=wb, want=want, bound=_bound(ca, sa, cb, sb, want), q=(ca, sa, cb, sb))


def _queries(case, dev):
    return {"feat_t": case["fa"].to(dev), "mask": case["mask"].to(dev), "weight": case["wa"].to(dev)}


def _fp8_index(case, dev):
    from valor_amd.search import RetrievalIndex
    return RetrievalIndex.from_features(case["fb"].to(dev), case["wb"].to(dev), [f"c{j}" for j in range(NB)], group="tv", bank_dtype="fp8")


@pytest.mark.parametrize("chunk", [64, 257, 700])
def test_index_search_equals_topk_of_its_scores(dev, fine_case, chunk):
    from valor_amd.search import topk_host
    index, q = _fp8_index(fine_case, dev), _queries(fine_case, dev)
    assert index.bank_dtype == "fp8" and index.dtype == torch.bfloat16 and index.feats[0].dtype == torch.uint8
    assert index.bank_bytes() == NB * NV * (D + 8) and index.fingerprint()["bank_dtype"] == "fp8_e4m3"
    res = index.search(None, q, TOPK, chunk=chunk)
    full = index.scores(None, q, chunk=chunk)
    want_v, want_i = topk_host(full.cpu(), TOPK)
    assert torch.equal(res.indices.cpu(), want_i) and torch.equal(res.scores.cpu(), want_v)
    assert res.ids == [[f"c{j}" for j in row] for row in want_i.tolist()]


def test_index_scores_equal_the_host_law(dev, fine_case):
    index, q = _fp8_index(fine_case, dev), _queries(fine_case, dev)
    assert torch.equal(index.feats[0].cpu(), fine_case["q"][2]) and torch.equal(index.scales[0].cpu(), fine_case["q"][3])
    for chunk in (None, 257):
        err = (index.scores(None, q, chunk=chunk).cpu().double() - fine_case["want"]).abs()
        print(f"chunk {chunk}: largest |index score - host law| {float(err.max()):.3g}, largest ratio to the bound {float((err / fine_case['bound']).max()):.3g}")
        assert bool((err <= fine_case["bound"]).all())
    q32 = dict(q, feat_t=q["feat_t"].float())                           # fp32 queries of the same values: the same codes, the same scores
    assert torch.equal(index.scores(None, q32), index.scores(None, q))


def test_add_features_in_pieces_and_quantize_give_the_same_bank(dev, fine_case):
    from valor_amd.search import RetrievalIndex
    whole, q = _fp8_index(fine_case, dev), _queries(fine_case, dev)
    fb, ws = fine_case["fb"].to(dev), whole.weights[0]
    ids = [f"c{j}" for j in range(NB)]
    cuts = (0, 300, 301, NB)
    pieces = RetrievalIndex.from_features(fb[:300], ws[:300].clone(), ids[:300], group="tv", weights_softmaxed=True, bank_dtype="fp8")
    for a, b in zip(cuts[1:-1], cuts[2:]):
        pieces.add_features([fb[a:b]], [ws[a:b]], ids[a:b])
    bf16 = RetrievalIndex.from_features(fb, fine_case["wb"].to(dev), ids, group="tv")
    again = bf16.quantize()
    assert bf16.bank_dtype is None and bf16.feats[0].dtype == torch.bfloat16 and "bank_dtype" not in bf16.fingerprint()
    want = whole.scores(None, q)
    for other in (pieces, again):
        assert len(other) == NB and other.ids == ids and other.fingerprint() == whole.fingerprint()
        assert torch.equal(other.feats[0], whole.feats[0]) and torch.equal(other.scales[0], whole.scales[0])
        assert torch.equal(other.weights[0], whole.weights[0]) and torch.equal(other.scores(None, q), want)


def test_fine_late_fusion_bank(dev, fine_case):
    """two parts with unit token weights: the sum of the two parts' host-law scores, within the two parts' bounds added"""
    from valor_amd.search import RetrievalIndex, fp8_scores_host, quantize_rows_host, topk_host
    fv, fa = fine_case["fb"][:, :6].contiguous(), fine_case["fb"][:, 6:].contiguous()
    index = RetrievalIndex.from_features([fv.to(dev), fa.to(dev)], group="tva", late_fusion=True, bank_dtype="fp8")
    q = {"feat_t": fine_case["fa"].to(dev), "mask": fine_case["mask"].to(dev)}
    ca, sa = fine_case["q"][:2]
    mask = fine_case["mask"]
    want, bound = 0.0, 0.0
    for f in (fv, fa):
        cb, sb = quantize_rows_host(f)
        ones = torch.ones(f.shape[:2])
        part = fp8_scores_host(ca, sa, cb, sb, mask, ones, _soft(torch.ones_like(mask), mask), _soft(ones, ones))
        want, bound = want + part, bound + _bound(ca, sa, cb, sb, part)
    full = index.scores(None, q, chunk=257)
    err = (full.cpu().double() - want).abs()
    print(f"largest |late-fusion score - host law| {float(err.max()):.3g}, largest ratio to the bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    res = index.search(None, q, TOPK, chunk=257)
    want_v, want_i = topk_host(full.cpu(), TOPK)
    assert torch.equal(res.indices.cpu(), want_i) and torch.equal(res.scores.cpu(), want_v)


# ------------------------------------------------------------------ 6. planted matches
@pytest.mark.parametrize("D", [128, 512])
def test_planted_clips_rank_first(dev, D):
    """query i is a noisy copy of clip 17 i % 300. On the host law alone every planted clip is first with a margin of at least 0.68
    against a largest fp8-vs-bf16 score difference of 5.4e-3; the fp8 index and the bf16 index must both return it, for all 16 queries."""
    from valor_amd.search import RetrievalIndex
    nb, nv, nq, t = 300, 10, 16, 12
    g = torch.Generator().manual_seed(0)
    clips = _unit(torch.randn((nb, nv, D), generator=g)).bfloat16()
    planted = torch.arange(nq) * 17 % nb
    noise = 0.5 * torch.randn((nq, t, D), generator=g) / D ** 0.5
    query = _unit(clips[planted].float()[:, torch.arange(t) % nv] + noise).bfloat16()
    wa, wb = torch.randn((nq, t), generator=g), torch.randn((nb, nv), generator=g)
    q = {"feat_t": query.to(dev), "weight": wa.to(dev)}
    bf16 = RetrievalIndex.from_features(clips.to(dev), wb.to(dev), group="tv")
    fp8 = RetrievalIndex.from_features(clips.to(dev), wb.to(dev), group="tv", bank_dtype="fp8")
    diff = (fp8.scores(None, q) - bf16.scores(None, q)).abs().max()
    two = fp8.search(None, q, 2).scores
    print(f"D {D}: largest |fp8 - bf16| score {float(diff):.3g}, smallest top-1 margin on the fp8 bank {float((two[:, 0] - two[:, 1]).min()):.3g}")
    for index in (fp8, bf16):
        assert index.search(None, q, 1).indices[:, 0].cpu().tolist() == planted.tolist()


# ------------------------------------------------------------------ 7. a model-built index
def _batches(spec, seed0, n_batches, clips=4):
    from valor_amd import synth
    out = []
    for i in range(n_batches):
        b = synth.make_batch(spec, batch=clips, frames=2, audio_slices=1, txt_len=32, seed=seed0 + i, bf16_exact=True)
        b["ids"] = [f"v{clips * i + j}" for j in range(clips)]
        out.append(b)
    return out


def test_index_built_by_a_model(dev, tmp_path):
    """the tiny spec and batches of tests/test_search_gpu.py::test_index_built_by_a_model, bf16"""
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    from valor_amd.search import RetrievalIndex
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05, bf16_exact=True)
    batches = _batches(spec, 70, 3)
    model = VALOR({"dropout": 0.0}, spec=spec, dtype=torch.bfloat16, device=dev)
    model.load_state_dict(sd, strict=True)
    model.eval()
    index = RetrievalIndex.build(model, batches, "tva", bank_dtype="fp8")
    assert len(index) == 12 and index.ids == [f"v{j}" for j in range(12)] and index.bank_dtype == "fp8" and index.dtype == torch.bfloat16
    queries = {"clip_tokens": torch.cat([b["txt_tokens"]["clip_tokens"] for b in batches], 0),
               "bert_tokens": torch.cat([b["txt_tokens"]["bert_tokens"] for b in batches], 0)}
    res = index.search(model, queries, 5)
    assert res.scores.shape == (12, 5) and bool(torch.isfinite(res.scores).all()) and all(i in index.ids for row in res.ids for i in row)
    index.save(tmp_path / "bank8.pt")
    back = RetrievalIndex.load(tmp_path / "bank8.pt", dev)
    again = back.search(model, queries, 5)
    assert back.fingerprint() == index.fingerprint() and back.bank_dtype == "fp8"
    assert torch.equal(again.scores, res.scores) and torch.equal(again.indices, res.indices) and again.ids == res.ids
    same = RetrievalIndex.build(model, batches, "tva").quantize()       # the bf16 index of the same batches, quantised afterwards
    for a, b in zip(same.feats + same.scales + same.weights, index.feats + index.scales + index.weights):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 8. refusals on the device
def test_a_non_finite_row_is_refused_and_nothing_is_appended(dev, fine_case):
    from valor_amd.search import RetrievalIndex, quantize_rows
    fb = fine_case["fb"][:40].to(dev)
    index = RetrievalIndex.from_features(fb, None, group="tv", bank_dtype="fp8")
    before = index.feats[0].clone()
    for poison in (float("nan"), float("inf")):
        rows = fb[:4].clone()
        rows[2, 3, 5] = poison
        with pytest.raises(ValueError, match="non-finite"):
            index.add_features([rows], [index.weights[0][:4]], ["x"] * 4)
        with pytest.raises(ValueError, match="non-finite"):
            quantize_rows(rows)
    assert len(index) == 40 and index.feats[0].shape[0] == 40 and torch.equal(index.feats[0], before) and index.scales[0].shape[0] == 40
    with pytest.raises(ValueError):                                     # queries of another width
        index.search(None, {"feat_t": torch.zeros((2, 12, 256), dtype=torch.bfloat16, device=dev)}, 5)
