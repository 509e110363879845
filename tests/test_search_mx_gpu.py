"""The MXFP4 clip bank on the GPU (csrc/search_mx.hip, search.RetrievalIndex with bank_dtype="mxfp4").

valor_mx_quantize_rows is held to mx_quantize_rows_host bit for bit. The operand layout of the block-scaled MFMA (which lane holds which
32 elements, which nibble comes first, whose scale byte is applied) is pinned by an EXACT case: inputs whose every partial sum is exact in
fp32 and for which any exchange of k positions, nibbles, blocks or scale bytes changes an answer. valor_fine_fused_fwd_mx is then held to
mx_scores_host (fp64) on the same codes inside a derived bound per (text, clip) pair:
    D * 2^-23 * max_{t,v}( sum_d |a_d b_d| )  +  8 * 2^-24 * |score|                  (a, b: the dequantised rows)
Products of an e4m3 and an e2m1 value are exact in fp32 and so are the power-of-two scales, so the first term covers D fp32 additions in
any order with unit roundoff 2^-23 (the MFMA's internal rounding is not documented as round-to-nearest); the second covers the weighted
token sums. On unit-norm rows this is some 1e-5, hundreds of times below the quantisation error: a wrong operand, scale or slot cannot
hide in it. The index is then held to its own kernel (exactly), to the exact bf16 search through its store, and to planted matches."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

E4M3, E2M1 = 0, 4


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _soft(raw, mask):
    return torch.softmax(raw.masked_fill(mask == 0, float("-inf")), dim=-1)


def _kernel(dev, ca, sa, cb, sb, maskA, maskB, wA, wB):
    """valor_fine_fused_fwd_mx on CPU tensors: fp32 [NA, NB] on the device"""
    from valor_amd import kernels as K, lib
    NA, T, D = ca.shape
    NB, Nv = cb.shape[:2]
    d = [t.to(dev).contiguous() for t in (ca, sa, cb, sb, maskA.float(), maskB.float(), wA.float(), wB.float())]
    out = torch.full((NA, NB), float("nan"), device=dev)
    lib.call("valor_fine_fused_fwd_mx", K._stream(), *[t.data_ptr() for t in d], out.data_ptr(), NA, NB, T, Nv, D)
    return out


# ------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("fmt", [E2M1, E4M3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantiser_equals_the_host_law_bit_for_bit(dev, dtype, fmt):
    from valor_amd.search import mx_quantize_rows, mx_quantize_rows_host
    g = torch.Generator().manual_seed(7)
    for rows in (1, 5, 257):
        for cols in (32, 128, 512):
            # blocks of very different magnitude (2^-12 .. 2^12); a zero row and a tiny row where there is room
            x = torch.randn((rows, cols), generator=g) * torch.exp2(torch.randint(-12, 13, (rows, cols // 32), generator=g).float()).repeat_interleave(32, dim=1)
            if rows > 2:
                x[1] = 0.0
                x[2] *= 2.0 ** -120
            x = x.to(dtype)
            want_c, want_s = mx_quantize_rows_host(x, fmt)
            got_c, got_s = mx_quantize_rows(x.to(dev), fmt)
            assert got_c.dtype == torch.uint8 and got_s.dtype == torch.uint8 and got_c.shape == want_c.shape and got_s.shape == want_s.shape
            assert torch.equal(got_s.cpu(), want_s), (rows, cols)
            assert torch.equal(got_c.cpu(), want_c), (rows, cols, int((got_c.cpu() != want_c).sum()))
    wide = (torch.randn((5, 160), generator=g) * 3).to(dtype).to(dev)   # ld = 160 > cols = 128: a column slice of a wider matrix
    view = wide[:, :128]
    assert not view.is_contiguous()
    got_c, got_s = mx_quantize_rows(view, fmt)
    want_c, want_s = mx_quantize_rows_host(view.cpu(), fmt)
    assert got_c.is_contiguous() and torch.equal(got_c.cpu(), want_c) and torch.equal(got_s.cpu(), want_s)
    three = torch.randn((3, 4, 64), generator=g).to(dtype)              # leading dimensions are kept
    got_c, got_s = mx_quantize_rows(three.to(dev), fmt)
    assert got_c.shape == (3, 4, 64 if fmt == E4M3 else 32) and got_s.shape == (3, 4, 2)
    assert torch.equal(got_c.cpu(), mx_quantize_rows_host(three, fmt)[0]) and torch.equal(got_s.cpu(), mx_quantize_rows_host(three, fmt)[1])


@pytest.mark.parametrize("fmt", [E2M1, E4M3])
def test_quantiser_on_the_hand_made_rows(dev, fmt):
    """the blocks of tests/test_search_mx_cpu.py: every e2m1 tie, the clamp, the sign of zero, zero and tiny blocks, e4m3 subnormals"""
    from test_search_mx_cpu import hand_rows
    from valor_amd.search import mx_quantize_rows
    x, want_codes, want_scales = hand_rows(fmt)
    codes, scales = mx_quantize_rows(x.to(dev), fmt)
    for i in range(x.shape[0]):
        assert codes[i].cpu().tolist() == want_codes[i].tolist(), (i, [hex(c) for c in codes[i].cpu().tolist()])
        assert scales[i].cpu().tolist() == want_scales[i].tolist(), (i, scales[i].cpu().tolist())
    # the same blocks side by side in ONE row: a block's neighbours do not leak into it
    row = x.reshape(1, -1)
    codes, scales = mx_quantize_rows(row.to(dev), fmt)
    assert torch.equal(codes.cpu(), want_codes.reshape(1, -1)) and torch.equal(scales.cpu(), want_scales.reshape(1, -1))


# ------------------------------------------------------------------ 2. the operand layout, exactly
_PJ = (5 * torch.arange(16) + 3) % 16


def _layout_case(D):
    """T = Nv = 1 and 16 x 16 rows, so score[i, j] is the bare contraction sum_k A[i, k] B[j, k]. With m = k // 16 and blk = k // 32:
        A[i, k] = 2^(m + 18 blk + i - 70) where k % 16 == i, else 0   e4m3 element 2^(m - blk) in {1, 2} * 2^blk, scale exponent 19 blk + i - 70
        B[j, k] = (1 or 1.5) * 2^(-18 blk + p(j) + 60)                 e2m1 element {1, 1.5} * 2^(blk % 3), exponent -18 blk + p(j) - blk % 3 + 60
    with p(j) = (5 j + 3) mod 16 a permutation (so the text's and the bank's scale bytes cannot stand in for each other) and
    B[j, k] having the 1.5 exactly when bit j of c(k) = (40503 k + 12345) mod 2^16 is set: c is injective, so the 16 clips spell out a
    different word for every k. Then score[i, j] = 2^(i + p(j) - 10) * sum_m 2^m (1 + bit / 2): a binary number of at most 18 bits that
    reads back, digit by digit, WHICH k of the bank met the text's m-th element. Every scale byte is unique in its tensor, and no two
    code blocks of a row are alike."""
    nblk, k = D // 32, torch.arange(D)
    m, blk = k // 16, k // 32
    ea = torch.where((k % 16)[None] == torch.arange(16)[:, None], torch.exp2((m - blk).float())[None], torch.zeros(())).view(16, 1, D)
    ca = ea.to(torch.float8_e4m3fn).view(torch.uint8)
    sa = (19 * torch.arange(nblk)[None] + torch.arange(16)[:, None] - 70 + 127).to(torch.uint8).view(16, 1, nblk)
    bits = ((((40503 * k + 12345) % 65536)[None] >> torch.arange(16)[:, None]) & 1)                      # [j, k]
    nib = ((2 + bits) + 2 * (blk % 3)[None]).to(torch.uint8)            # codes 2, 3 = 1, 1.5; 4, 5 = 2, 3; 6, 7 = 4, 6
    cb = (nib[:, 0::2] | (nib[:, 1::2] << 4)).view(16, 1, D // 2)
    sb = (-18 * torch.arange(nblk)[None] + _PJ[:, None] - (torch.arange(nblk) % 3)[None] + 60 + 127).to(torch.uint8).view(16, 1, nblk)
    return ca, sa, cb, sb


@pytest.mark.parametrize("D", [128, 256])
def test_operand_layout_of_the_scaled_mfma_exactly(dev, D):
    from valor_amd.search import mx_dequantize_host, mx_scores_host
    ca, sa, cb, sb = _layout_case(D)
    one = torch.ones((16, 1))
    law = lambda ca, sa, cb, sb: mx_scores_host(ca, sa, cb, sb, one, one, one, one)
    want = law(ca, sa, cb, sb)
    # ---- the properties of the inputs, checked here on the CPU
    a, b = mx_dequantize_host(ca, sa, E4M3)[:, 0], mx_dequantize_host(cb, sb, E2M1)[:, 0]
    assert bool(((a != 0).sum(0) == 1).all()) and bool((b != 0).all())                               # every k meets exactly one text
    grain = torch.exp2(torch.arange(16).double()[:, None] + _PJ.double()[None] - 11)                 # every term is a multiple of it
    total = torch.einsum("ik,jk->ij", a.abs(), b.abs()) / grain
    assert bool((total == total.round()).all()) and bool((total < 2 ** 24).all())                  # any partial sum is exact in fp32
    assert torch.equal(want, torch.einsum("ik,jk->ij", a, b)) and torch.equal(want.float().double(), want)
    for s in (sa, sb):
        assert s.unique().numel() == s.numel() and int(s.max()) < 255                               # no two scale bytes alike
    swap = lambda t, dim, p, q: t.index_select(dim, torch.tensor([q if x == p else p if x == q else x for x in range(t.shape[dim])]))
    wrong = {
        "two k of the text rows, one block": (swap(ca, 2, 3, 19), sa, cb, sb),
        "two k of the text rows, neighbours": (swap(ca, 2, 40, 41), sa, cb, sb),
        "two k of the text rows, two blocks": (swap(ca, 2, 5, 102), sa, cb, sb),
        "the nibbles of every bank byte": (ca, sa, (cb >> 4) | (cb << 4), sb),
        "two bytes of the bank rows": (ca, sa, swap(cb, 2, 7, 9), sb),
        "two 16-byte halves of a text block": (swap(ca.view(16, 1, D // 16, 16), 2, 0, 1).reshape(ca.shape), sa, cb, sb),
        "two blocks of the bank codes": (ca, sa, swap(cb.view(16, 1, D // 32, 16), 2, 1, 2).reshape(cb.shape), sb),
        "two blocks of the text codes": (swap(ca.view(16, 1, D // 32, 32), 2, 0, 3).reshape(ca.shape), sa, cb, sb),
        "two scale bytes of the text rows": (ca, swap(sa, 2, 0, 1), cb, sb),
        "two scale bytes of the bank rows": (ca, sa, cb, swap(sb, 2, 2, 3)),
        "the next row's text scales": (ca, sa.roll(1, 0), cb, sb),
        "the next row's bank scales": (ca, sa, cb, sb.roll(1, 0)),
        "the next block's text scales": (ca, sa.roll(1, 2), cb, sb),
        "the next block's bank scales": (ca, sa, cb, sb.roll(1, 2)),
        "text and bank scales exchanged": (ca, sb, cb, sa),
    }
    for name, case in wrong.items():
        assert not torch.equal(law(*case), want), name
    # ---- the device
    got = _kernel(dev, ca, sa, cb, sb, one, one, one, one).cpu().double()
    bad = (got != want).nonzero().tolist()
    assert not bad, (len(bad), bad[:4], [(got[i, j].item().hex(), want[i, j].item().hex()) for i, j in bad[:4]])


# ------------------------------------------------------------------ 3. the score kernel
def _bound(ca, sa, cb, sb, want):
    """the per-pair tolerance of the module docstring, in fp64 on the CPU"""
    from valor_amd.search import mx_dequantize_host
    mag = torch.einsum("atd,bvd->abtv", mx_dequantize_host(ca, sa, E4M3).abs(), mx_dequantize_host(cb, sb, E2M1).abs())
    return ca.shape[-1] * 2.0 ** -23 * mag.amax(dim=(2, 3)) + 8 * 2.0 ** -24 * want.abs()


def _score_case(NA, NB, T, Nv, D, seed, spread=0):
    """unit rows (spread: every block of 32 further scaled by 2^-spread .. 2^spread), the fp8 test's length masks with one text of a
    single live token; returns the host-quantised operands and the fp64 scores of the UNquantised rows"""
    from valor_amd.search import mx_quantize_rows_host
    g = torch.Generator().manual_seed(seed)
    fa, fb = _unit(torch.randn((NA, T, D), generator=g)), _unit(torch.randn((NB, Nv, D), generator=g))
    if spread:
        fa = fa * torch.exp2(torch.randint(-spread, spread + 1, (NA, T, D // 32), generator=g).float()).repeat_interleave(32, dim=2)
        fb = fb * torch.exp2(torch.randint(-spread, spread + 1, (NB, Nv, D // 32), generator=g).float()).repeat_interleave(32, dim=2)
    ca, sa = mx_quantize_rows_host(fa, E4M3)
    cb, sb = mx_quantize_rows_host(fb, E2M1)
    lens = torch.randint(1, T + 1, (NA,), generator=g)
    lens[NA // 2] = 1                                                   # one text with a single live token
    maskA = (torch.arange(T)[None] < lens[:, None]).float()
    maskB = torch.ones((NB, Nv))
    wA, wB = _soft(torch.randn((NA, T), generator=g), maskA), _soft(torch.randn((NB, Nv), generator=g), maskB)
    x = torch.einsum("atd,bvd->abtv", fa.double(), fb.double()) * maskA.double()[:, None, :, None]
    exact = (torch.einsum("abt,at->ab", x.max(dim=3)[0], wA.double()) + torch.einsum("abv,bv->ab", x.max(dim=2)[0], wB.double())) / 2.0
    return (ca, sa, cb, sb, maskA, maskB, wA, wB), exact


@pytest.mark.parametrize("NA,NB,T,Nv,D,spread", [(1, 1, 1, 1, 128, 0), (3, 5, 7, 10, 128, 0), (9, 17, 32, 10, 512, 0), (5, 9, 33, 17, 256, 0),
                                                 (2, 3, 64, 64, 128, 0), (70, 130, 12, 10, 128, 0), (9, 17, 12, 10, 256, 10)])
def test_score_kernel_against_the_host_law(dev, NA, NB, T, Nv, D, spread):
    from valor_amd.search import mx_scores_host
    case, exact = _score_case(NA, NB, T, Nv, D, seed=NA * 1000 + NB, spread=spread)
    want = mx_scores_host(*case)
    bound = _bound(case[0], case[1], case[2], case[3], want)
    quant = float((want - exact).abs().max())
    got = _kernel(dev, *case).cpu().double()
    err = (got - want).abs()
    print(f"largest |kernel - host law| {float(err.max()):.3g}; bound {float(bound.min()):.3g} .. {float(bound.max()):.3g}; "
          f"largest ratio {float((err / bound).max()):.3g}; quantisation error of the case {quant:.3g}")
    assert 100 * float(bound.max()) <= quant                            # nothing wrong can hide in the bound
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ 4. the index equals its own kernel and law
NB, NV, T, D, NQ, TOPK = 1000, 10, 12, 128, 9, 20


@pytest.fixture(scope="module")
def fine_case():
    """bf16 unit features, text masks of random length, raw token weights, and the host-quantised rows (once)"""
    from valor_amd.search import mx_quantize_rows_host
    g = torch.Generator().manual_seed(11)
    fb = _unit(torch.randn((NB, NV, D), generator=g)).bfloat16()
    fa = _unit(torch.randn((NQ, T, D), generator=g)).bfloat16()
    mask = (torch.arange(T)[None] < torch.randint(3, T + 1, (NQ, 1), generator=g)).float()
    wa, wb = torch.randn((NQ, T), generator=g), torch.randn((NB, NV), generator=g)
    return dict(fa=fa, fb=fb, mask=mask, wa=wa, wb=wb, q=mx_quantize_rows_host(fa, E4M3) + mx_quantize_rows_host(fb, E2M1))


def _queries(case, dev):
    return {"feat_t": case["fa"].to(dev), "mask": case["mask"].to(dev), "weight": case["wa"].to(dev)}


def _ids(n=NB):
    return [f"c{j}" for j in range(n)]


def _mx_index(case, dev, n=NB, exact=None):
    from valor_amd.search import RetrievalIndex
    return RetrievalIndex.from_features(case["fb"][:n].to(dev), case["wb"][:n].to(dev), _ids(n), group="tv", bank_dtype="mxfp4", exact=exact)


def test_index_scores_equal_its_kernel_on_host_quantised_rows(dev, fine_case):
    from valor_amd import kernels as K, lib
    from valor_amd.search import mx_scores_host
    index, q = _mx_index(fine_case, dev), _queries(fine_case, dev)
    ca, sa, cb, sb = fine_case["q"]
    assert index.bank_dtype == "mxfp4" and index.dtype == torch.bfloat16 and index.dim == D and index.fingerprint()["bank_dtype"] == "mxfp4_e2m1"
    assert torch.equal(index.feats[0].cpu(), cb) and torch.equal(index.scales[0].cpu(), sb)
    ones = torch.ones((NB, NV))
    wB = _soft(fine_case["wb"], ones)
    assert torch.allclose(index.weights[0].cpu(), wB, rtol=1e-5, atol=1e-8)
    # the text weights as the index makes them (valor_fine_weight_softmax), so that the comparison below can be exact
    raw, msk, wA = fine_case["wa"].to(dev).contiguous(), fine_case["mask"].to(dev).contiguous(), torch.empty((NQ, T), device=dev)
    lib.call("valor_fine_weight_softmax", K._stream(), raw.data_ptr(), msk.data_ptr(), wA.data_ptr(), NQ, T)
    wA = wA.cpu()
    assert torch.allclose(wA, _soft(fine_case["wa"], fine_case["mask"]), rtol=1e-5, atol=1e-8)
    direct = _kernel(dev, ca, sa, cb, sb, fine_case["mask"], ones, wA, index.weights[0].cpu())
    for chunk in (None, 64, 257, 700):
        assert torch.equal(index.scores(None, q, chunk=chunk), direct), chunk
    want = mx_scores_host(ca, sa, cb, sb, fine_case["mask"], ones, wA, index.weights[0].cpu())
    err = (direct.cpu().double() - want).abs()
    bound = _bound(ca, sa, cb, sb, want)
    print(f"largest |index score - host law| {float(err.max()):.3g}, largest ratio to the bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    q32 = dict(q, feat_t=q["feat_t"].float())                           # fp32 queries of the same values: the same codes, the same scores
    assert torch.equal(index.scores(None, q32), direct)


@pytest.mark.parametrize("chunk", [64, 257, 700])
def test_index_search_equals_topk_of_its_scores(dev, fine_case, chunk):
    from valor_amd.search import topk_host
    index, q = _mx_index(fine_case, dev), _queries(fine_case, dev)
    res = index.search(None, q, TOPK, chunk=chunk)
    want_v, want_i = topk_host(index.scores(None, q, chunk=chunk).cpu(), TOPK)
    assert torch.equal(res.indices.cpu(), want_i) and torch.equal(res.scores.cpu(), want_v)
    assert res.ids == [[f"c{j}" for j in row] for row in want_i.tolist()]


def test_add_in_pieces_quantize_and_files_give_the_same_bank(dev, fine_case, tmp_path):
    from valor_amd.search import RetrievalIndex
    whole, q = _mx_index(fine_case, dev, exact="device"), _queries(fine_case, dev)
    fb, ws, ids = fine_case["fb"].to(dev), whole.weights[0], _ids()
    pieces = RetrievalIndex.from_features(fb[:300], ws[:300].clone(), ids[:300], group="tv", weights_softmaxed=True, bank_dtype="mxfp4", exact="device")
    for a, b in ((300, 301), (301, NB)):
        pieces.add_features([fb[a:b]], [ws[a:b]], ids[a:b])
    bf16 = RetrievalIndex.from_features(fb, fine_case["wb"].to(dev), ids, group="tv")
    again = bf16.quantize(bank_dtype="mxfp4", exact="device")
    assert bf16.quantize().bank_dtype == "fp8"                          # the default stays
    want = whole.scores(None, q)
    for other in (pieces, again):
        assert len(other) == NB and other.ids == ids and other.fingerprint() == whole.fingerprint() and other.bank_bytes() == whole.bank_bytes()
        assert torch.equal(other.feats[0], whole.feats[0]) and torch.equal(other.scales[0], whole.scales[0])
        assert torch.equal(other.exact_feats[0], fb) and torch.equal(other.weights[0], whole.weights[0]) and torch.equal(other.scores(None, q), want)
    res = whole.search(None, q, TOPK)
    plain = _mx_index(fine_case, dev)
    for index, tag in ((plain, "/4"), (whole, "/5")):
        path = tmp_path / f"bank{tag[1]}.pt"
        index.save(path)
        assert torch.load(path, map_location="cpu", weights_only=True)["format"] == "valor_amd.RetrievalIndex" + tag
        back = RetrievalIndex.load(path, dev)
        assert back.bank_dtype == "mxfp4" and back.exact == index.exact and back.fingerprint() == index.fingerprint() and back.ids == ids
        for a, b in zip(back.feats + back.scales + back.weights + (back.exact_feats or []), index.feats + index.scales + index.weights + (index.exact_feats or [])):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert torch.equal(back.scores(None, q), want)
    again = RetrievalIndex.load(tmp_path / "bank5.pt", dev).search(None, q, TOPK)
    assert torch.equal(again.scores, res.scores) and torch.equal(again.indices, res.indices)


# ------------------------------------------------------------------ 5. the two-stage search
@pytest.mark.parametrize("exact", ["device", "host"])
def test_two_stage_search_returns_the_exact_answer(dev, fine_case, exact):
    from valor_amd.search import RetrievalIndex
    n = 200                                                             # at most 256 clips: the shortlist can hold the whole bank
    q = _queries(fine_case, dev)
    bf16 = RetrievalIndex.from_features(fine_case["fb"][:n].to(dev), fine_case["wb"][:n].to(dev), _ids(n), group="tv")
    index, plain = _mx_index(fine_case, dev, n, exact=exact), _mx_index(fine_case, dev, n)
    want = bf16.search(None, q, TOPK)
    got = index.search(None, q, TOPK, shortlist=256)
    assert torch.equal(got.indices, want.indices) and torch.equal(got.scores, want.scores)
    assert torch.equal(index.rescore(None, q, want.indices), want.scores)
    within = index.search(None, q, 5, within=want.indices)
    assert torch.equal(within.indices, want.indices[:, :5]) and torch.equal(within.scores, want.scores[:, :5])
    fp4 = index.search(None, q, TOPK, shortlist=0)                       # the fp4 scores alone: what an index without a store returns
    alone = plain.search(None, q, TOPK)
    assert torch.equal(fp4.indices, alone.indices) and torch.equal(fp4.scores, alone.scores)
    assert not torch.equal(fp4.scores, want.scores)
    default = index.search(None, q, 5)                                   # the default shortlist is a two-stage search
    assert bool((default.scores == index.rescore(None, q, default.indices)).all())
    al = index.explain(None, q, want.indices[:, :3])
    assert torch.equal(al.parts[0].score, want.scores[:, :3])
    cand = want.indices[:, :3].contiguous()
    with pytest.raises(ValueError, match="exact store"):
        plain.search(None, q, 5, shortlist=20)
    with pytest.raises(ValueError, match="exact store"):
        plain.rescore(None, q, cand)
    with pytest.raises(ValueError, match="exact store"):
        plain.explain(None, q, cand)


# ------------------------------------------------------------------ 6. planted matches
def _planted(Dp):
    """the construction of tests/test_search_fp8_gpu.py: query i is a noisy copy of clip 17 i % 300"""
    nb, nv, nq, t = 300, 10, 16, 12
    g = torch.Generator().manual_seed(0)
    clips = _unit(torch.randn((nb, nv, Dp), generator=g)).bfloat16()
    planted = torch.arange(nq) * 17 % nb
    noise = 0.5 * torch.randn((nq, t, Dp), generator=g) / Dp ** 0.5
    query = _unit(clips[planted].float()[:, torch.arange(t) % nv] + noise).bfloat16()
    wa, wb = torch.randn((nq, t), generator=g), torch.randn((nb, nv), generator=g)
    return clips, query, wa, wb, planted


@pytest.mark.parametrize("Dp", [128, 512])
def test_planted_clips_rank_first(dev, Dp):
    """On the host law alone every planted clip is first with a margin of at least 0.66 against a largest mxfp4-vs-exact score
    difference of at most 0.04 (asserted here, on the CPU); the mxfp4 index must return every planted clip first, with no re-scoring."""
    from valor_amd.search import RetrievalIndex, mx_quantize_rows_host, mx_scores_host
    clips, query, wa, wb, planted = _planted(Dp)
    ones_a, ones_b = torch.ones(query.shape[:2]), torch.ones(clips.shape[:2])
    sA, sB = _soft(wa, ones_a), _soft(wb, ones_b)
    law = mx_scores_host(*mx_quantize_rows_host(query, E4M3), *mx_quantize_rows_host(clips, E2M1), ones_a, ones_b, sA, sB)
    x = torch.einsum("atd,bvd->abtv", query.double(), clips.double())
    exact = (torch.einsum("abt,at->ab", x.max(dim=3)[0], sA.double()) + torch.einsum("abv,bv->ab", x.max(dim=2)[0], sB.double())) / 2.0
    two = law.topk(2, dim=1)
    margin, error = float((two.values[:, 0] - two.values[:, 1]).min()), float((law - exact).abs().max())
    print(f"D {Dp}, host law: smallest top-1 margin {margin:.3g}, largest |mxfp4 - exact| score {error:.3g}")
    assert two.indices[:, 0].tolist() == planted.tolist() and margin >= 0.66 and error <= 0.04
    q = {"feat_t": query.to(dev), "weight": wa.to(dev)}
    mx = RetrievalIndex.from_features(clips.to(dev), wb.to(dev), group="tv", bank_dtype="mxfp4")
    bf16 = RetrievalIndex.from_features(clips.to(dev), wb.to(dev), group="tv")
    diff = (mx.scores(None, q) - bf16.scores(None, q)).abs().max()
    top = mx.search(None, q, 2).scores
    print(f"D {Dp}, device: largest |mxfp4 - bf16| score {float(diff):.3g}, smallest top-1 margin on the mxfp4 bank {float((top[:, 0] - top[:, 1]).min()):.3g}")
    assert mx.search(None, q, 1).indices[:, 0].cpu().tolist() == planted.tolist()
    assert float(diff) <= 0.04 + 1e-3 and float((top[:, 0] - top[:, 1]).min()) >= 0.66 - 1e-3


# ------------------------------------------------------------------ 7. bytes
def test_bank_bytes(dev, fine_case):
    from valor_amd.search import RetrievalIndex
    mx = _mx_index(fine_case, dev)
    fp8 = RetrievalIndex.from_features(fine_case["fb"].to(dev), fine_case["wb"].to(dev), _ids(), group="tv", bank_dtype="fp8")
    assert mx.bank_bytes() == NB * NV * (D // 2 + D // 32 + 4)          # codes, scale bytes, fp32 token weights
    assert mx.bank_bytes() < 0.55 * fp8.bank_bytes()
    assert _mx_index(fine_case, dev, exact="host").bank_bytes() == mx.bank_bytes()                   # a host store costs no device bytes
    assert _mx_index(fine_case, dev, exact="device").bank_bytes() == mx.bank_bytes() + NB * NV * D * 2


# ------------------------------------------------------------------ 8. refusals on the device
def test_a_non_finite_row_is_refused_and_nothing_is_appended(dev, fine_case):
    from valor_amd.search import mx_quantize_rows
    fb = fine_case["fb"][:40].to(dev)
    index = _mx_index(fine_case, dev, 40, exact="device")
    before = index.feats[0].clone()
    for poison in (float("nan"), float("inf")):
        rows = fb[:4].clone()
        rows[2, 3, 5] = poison
        with pytest.raises(ValueError, match="non-finite"):
            index.add_features([rows], [index.weights[0][:4]], ["x"] * 4)
        with pytest.raises(ValueError, match="non-finite"):
            mx_quantize_rows(rows, E2M1)
    assert len(index) == 40 and torch.equal(index.feats[0], before) and index.scales[0].shape[0] == 40 and index.exact_feats[0].shape[0] == 40
    with pytest.raises(ValueError):                                     # rows of another width
        index.add_features([torch.zeros((2, NV, 256), dtype=torch.bfloat16, device=dev)], [index.weights[0][:2]], ["y"] * 2)
    with pytest.raises(ValueError):                                     # queries of another width
        index.search(None, {"feat_t": torch.zeros((2, 12, 256), dtype=torch.bfloat16, device=dev)}, 5)
