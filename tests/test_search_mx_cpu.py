"""The MXFP4 clip bank without a GPU: the OCP MX quantisation law on hand-made rows (expected code and scale bytes written out), the round
trip, nibble order and leading dimensions, the score law against the project's oracle on the dequantised rows, argument validation of the
two entry points, and the persistence / refusal rules on CPU tensors."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

E4M3, E2M1 = 0, 4                                                      # VALOR_MX_E4M3 / VALOR_MX_E2M1

# (leading elements of one block of 32, expected leading code BYTES, expected scale byte); the rest of the block is zero and so are its
# codes. Shared with tests/test_search_mx_gpu.py. e2m1 codes 0 .. 7 stand for 0, .5, 1, 1.5, 2, 3, 4, 6; bit 3 is the sign; element 2i is
# the low nibble of byte i.
HAND_BLOCKS_E2M1 = [
    # amax 5 -> e = 2, s = 0, byte 127. Every tie of the format goes to the even code: .25 -> 0 (code 0), .75 -> 1 (2), 1.25 -> 1 (2),
    # 1.75 -> 2 (4), 2.5 -> 2 (4), 3.5 -> 4 (6), 5 -> 4 (6); then the same with the sign bit
    ([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 4.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -4.0],
     [0x20, 0x42, 0x64, 0x66, 0xA8, 0xCA, 0xEC, 0xEE], 127),
    # just off the ties, on either side
    ([0.2500001, 0.7499999, 1.2500001, 1.7499999, 2.5000002, 3.4999998, 5.0000005, 4.0], [0x11, 0x33, 0x55, 0x67], 127),
    # saturation: amax 7 keeps s = 0 (e = 2) and 7 clamps to 6 (code 7)
    ([7.0, -7.0, 6.0, 1.0, 7.9999995, 0.0], [0xF7, 0x27, 0x07], 127),
    # the sign of zero is kept; amax 1 -> e = 0, s = -2, byte 125: 1 * 4 = 4 (code 6)
    ([-0.0, 0.0, 1.0, -1.0], [0x08, 0xE6], 125),
    # an all-zero block: byte 0, zero codes
    ([0.0, 0.0, 0.0, 0.0], [0x00, 0x00], 0),
    # amax exactly a power of two: 2 -> e = 1, s = -1, byte 126; 2, 1, .5, .25, .125 (a tie -> 0) become 4, 2, 1, .5, .25 -> codes 6, 4, 2, 1, 0
    ([2.0, 1.0, 0.5, 0.25, 0.125, -0.125], [0x46, 0x12, 0x80], 126),
    # ... and just below it: 1.9999999 -> e = 0, s = -2, byte 125; 1.9999999 * 4 = 7.9999995 clamps to 6
    ([1.9999999, 1.0, 0.5, 0.25], [0x67, 0x24], 125),
    # a tiny block: amax 2^-128 is an fp32 subnormal -> s = -127, byte 0; 2^-130 * 2^127 = .125 rounds to 0, -2^-128 * 2^127 = -.5 (code 9)
    ([2.0 ** -130, -(2.0 ** -128)], [0x90], 0),
]
S9 = 2.0 ** -9                                                         # the smallest e4m3 subnormal
HAND_BLOCKS_E4M3 = [
    # amax 256 = 2^8 exactly -> e = 8, s = 0, byte 127. Subnormal outputs (steps of 2^-9), ties to even (2^-10 -> 0, 1.5 -> 2, 2.5 -> 2),
    # the sign kept on a value that rounds to zero, 2^-6 the smallest normal
    ([256.0, S9, 3 * S9, S9 / 2, 1.5 * S9, -S9, 8 * S9, -S9 / 2, 2.5 * S9, S9 / 4, 1.0, -0.0],
     [0x78, 0x01, 0x03, 0x00, 0x02, 0x81, 0x08, 0x80, 0x02, 0x00, 0x38, 0x80], 127),
    # saturation: amax 500 keeps s = 0 and clamps to 448 = 0x7E, never NaN (0x7F); 464 is the tie between 448 and the missing 480
    ([500.0, -500.0, 448.0, 464.0, 511.99997], [0x7E, 0xFE, 0x7E, 0x7E, 0x7E], 127),
    # ties in the binade [16, 32) (steps of 2) under s = 0: 17 -> 16, 19 -> 20, 21 -> 20, 23 -> 24
    ([300.0, 17.0, 19.0, 21.0, 23.0, -17.0, -19.0], [0x79, 0x58, 0x5A, 0x5A, 0x5C, 0xD8, 0xDA], 127),
    # amax 1 -> e = 0, s = -8, byte 119: 1 -> 256 = 0x78, -.5 -> -128 = 0xF0, 2^-17 -> 2^-9 = 0x01
    ([1.0, -0.5, 2.0 ** -17, 0.0], [0x78, 0xF0, 0x01, 0x00], 119),
    # an all-zero block
    ([0.0, -0.0], [0x00, 0x80], 0),
    # a tiny block: s = -127, byte 0; 2^-127 * 2^127 = 1 = 0x38
    ([2.0 ** -127, 2.0 ** -130], [0x38, 0x20], 0),
]


def _block(head):
    return torch.tensor(list(head) + [0.0] * (32 - len(head)), dtype=torch.float32)


def hand_rows(fmt):
    """the hand-made blocks as a [blocks, 32] fp32 matrix, the expected codes [blocks, 32 or 16] and scale bytes [blocks, 1]"""
    table = HAND_BLOCKS_E2M1 if fmt == E2M1 else HAND_BLOCKS_E4M3
    x = torch.stack([_block(head) for head, _, _ in table])
    codes = torch.zeros((len(table), 16 if fmt == E2M1 else 32), dtype=torch.uint8)
    for i, (_, want, _) in enumerate(table):
        codes[i, :len(want)] = torch.tensor(want, dtype=torch.uint8)
    return x, codes, torch.tensor([[b] for _, _, b in table], dtype=torch.uint8)


# ------------------------------------------------------------------ 1. the quantisation law
@pytest.mark.parametrize("fmt", [E2M1, E4M3])
def test_mx_quantize_rows_host_on_hand_made_rows(fmt):
    from valor_amd.search import MX_E2M1, MX_E4M3, mx_quantize_rows_host
    assert (MX_E4M3, MX_E2M1) == (E4M3, E2M1)
    x, want_codes, want_scales = hand_rows(fmt)
    codes, scales = mx_quantize_rows_host(x, fmt)
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and codes.shape == want_codes.shape and scales.shape == want_scales.shape
    for i in range(x.shape[0]):
        assert codes[i].tolist() == want_codes[i].tolist(), (i, x[i, :16].tolist(), [hex(c) for c in codes[i].tolist()])
        assert scales[i].tolist() == want_scales[i].tolist(), (i, scales[i].tolist())
    assert not bool((scales == 255).any())


def test_two_blocks_of_one_row_far_apart_get_their_own_scales():
    """blocks of one row 2^20 apart: each gets its own exponent, and the same codes"""
    from valor_amd.search import mx_dequantize_host, mx_quantize_rows_host
    small = torch.tensor([3.0, -1.5, 1.0, 0.5] + [0.0] * 28)
    x = torch.cat((small, small * 2.0 ** 20, small * 2.0 ** -20))[None]
    codes, scales = mx_quantize_rows_host(x, E2M1)
    # amax 3 -> e = 1, s = -1, byte 126; 3, -1.5, 1, .5 become 6, -3, 2, 1 -> codes 7, 0xD, 4, 2
    assert scales.tolist() == [[126, 146, 106]]
    assert codes[0].view(3, 16)[:, :2].tolist() == [[0xD7, 0x24]] * 3 and not bool(codes[0].view(3, 16)[:, 2:].any())
    assert torch.equal(mx_dequantize_host(codes, scales, E2M1), x.double())
    codes, scales = mx_quantize_rows_host(x, E4M3)
    # e = 1, s = -7, byte 120; 3 * 128 = 384 = 0x7C, -192 = 0xF4, 128 = 0x70, 64 = 0x68
    assert scales.tolist() == [[120, 140, 100]]
    assert codes[0].view(3, 32)[:, :4].tolist() == [[0x7C, 0xF4, 0x70, 0x68]] * 3
    assert torch.equal(mx_dequantize_host(codes, scales, E4M3), x.double())


def _step(y, fmt):
    """the spacing of the element format at magnitude y"""
    e = torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -40)))
    return torch.pow(2.0, e.clamp(min=0.0) - 1.0) if fmt == E2M1 else torch.pow(2.0, e.clamp(min=-6.0) - 3.0)


@pytest.mark.parametrize("fmt", [E2M1, E4M3])
def test_round_trip_is_within_half_a_step_and_idempotent(fmt):
    from valor_amd.search import mx_dequantize_host, mx_quantize_rows_host
    g = torch.Generator().manual_seed(5)
    vmax = 6.0 if fmt == E2M1 else 448.0
    x = torch.randn((37, 256), generator=g) * torch.exp2(torch.randint(-12, 13, (37, 8), generator=g).float()).repeat_interleave(32, dim=1)
    codes, scales = mx_quantize_rows_host(x, fmt)
    back = mx_dequantize_host(codes, scales, fmt)
    assert back.dtype == torch.float64 and back.shape == x.shape
    two = torch.pow(2.0, scales.double() - 127.0).repeat_interleave(32, dim=1)
    y, yb = x.double() / two, back / two                                 # in units of the block's scale
    inside = y.abs() <= vmax
    assert bool((yb.abs() <= vmax).all()) and bool((yb[~inside].abs() == vmax).all())
    assert bool(((yb - y).abs()[inside] <= 0.5 * _step(y, fmt)[inside]).all())
    # the largest element of every block lands in the format's top binade: no bit of range is wasted, none overflows the scale
    top = yb.abs().view(37, 8, 32).amax(-1)
    assert bool((top >= (4.0 if fmt == E2M1 else 256.0)).all())
    # values already representable come back as they are, codes and scale bytes included
    c2, s2 = mx_quantize_rows_host(back.float(), fmt)
    assert torch.equal(back.float().double(), back) and torch.equal(c2, codes) and torch.equal(s2, scales)
    assert torch.equal(mx_dequantize_host(c2, s2, fmt), back)


def test_nibble_order_and_leading_dimensions():
    from valor_amd.search import E2M1_VALUES, mx_dequantize_host, mx_quantize_rows_host
    # element k of the row is the magnitude of code k % 8 (scaled so that amax 6 keeps s = 0): byte i holds codes (2i, 2i + 1) = (low, high)
    row = torch.tensor([E2M1_VALUES[k % 8] for k in range(32)])
    codes, scales = mx_quantize_rows_host(row[None], E2M1)
    assert scales.tolist() == [[127]] and codes[0].tolist() == [0x10, 0x32, 0x54, 0x76] * 4
    assert torch.equal(mx_dequantize_host(codes, scales, E2M1)[0], row.double())
    # leading dimensions are kept, bf16 input is widened exactly
    x = torch.randn((3, 5, 64), generator=torch.Generator().manual_seed(0)).bfloat16()
    for fmt, width in ((E2M1, 32), (E4M3, 64)):
        c3, s3 = mx_quantize_rows_host(x, fmt)
        c2, s2 = mx_quantize_rows_host(x.float().view(15, 64), fmt)
        assert c3.shape == (3, 5, width) and s3.shape == (3, 5, 2) and torch.equal(c3.view(15, width), c2) and torch.equal(s3.view(15, 2), s2)
        assert mx_dequantize_host(c3, s3, fmt).shape == (3, 5, 64)
    with pytest.raises(ValueError, match="multiple of 32"):
        mx_quantize_rows_host(torch.zeros((2, 48)), E2M1)
    with pytest.raises(ValueError, match="fmt"):
        mx_quantize_rows_host(torch.zeros((2, 32)), 2)


def test_mx_scores_host_against_the_oracle_on_dequantised_rows():
    """Oracle.compute_fine_matrix in fp32 on the dequantised rows, band 2e-5 + 1e-5 |s|: the new score law is the project's"""
    import valor_oracle as VO
    from valor_amd.search import mx_dequantize_host, mx_quantize_rows_host, mx_scores_host
    NA, NB, T, Nv, D = 5, 9, 7, 10, 128
    g = torch.Generator().manual_seed(3)
    fa, fb = torch.randn((NA, T, D), generator=g), torch.randn((NB, Nv, D), generator=g)
    ca, sa = mx_quantize_rows_host(fa, E4M3)
    cb, sb = mx_quantize_rows_host(fb, E2M1)
    maskA = (torch.arange(T)[None] < torch.tensor([7, 1, 4, 6, 2])[:, None]).long()
    maskB = torch.ones((NB, Nv), dtype=torch.long)
    maskB[2, 7:] = 0
    rawA, rawB = torch.randn((NA, T), generator=g), torch.randn((NB, Nv), generator=g)
    want = VO.Oracle.compute_fine_matrix(mx_dequantize_host(ca, sa, E4M3).float(), mx_dequantize_host(cb, sb, E2M1).float(), maskA, maskB, rawA, rawB)
    soft = lambda raw, m: torch.softmax(raw.masked_fill(m == 0, float("-inf")), dim=-1)
    got = mx_scores_host(ca, sa, cb, sb, maskA, maskB, soft(rawA, maskA), soft(rawB, maskB))
    assert got.dtype == torch.float64 and got.shape == (NA, NB)
    err = (got - want.double()).abs()
    print(f"largest |mx_scores_host - oracle| {float(err.max()):.3g}")
    assert bool((err <= 2e-5 + 1e-5 * want.double().abs()).all())


# ------------------------------------------------------------------ 2. the entry points' argument checks
def test_argument_validation_without_gpu():
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0

    def quant(x=p, ld=128, rows=4, cols=128, fmt=E2M1, codes=p, scales=p, dtype=0):
        return so.valor_mx_quantize_rows(None, dtype, x, ld, rows, cols, fmt, codes, scales)

    assert quant(x=None) == -1 and quant(codes=None) == -1 and quant(scales=None) == -1
    assert quant(cols=16) == -1 and quant(cols=0) == -1 and quant(cols=48) == -1 and quant(cols=-32) == -1
    for fmt in (1, 2, 3, 5, -1):
        assert quant(fmt=fmt) == -1, fmt
    assert quant(ld=64) == -1 and quant(dtype=7) == -1 and quant(x=p + 2) == -1 and quant(codes=p + 4) == -1 and quant(rows=-1) == -1
    assert quant(ld=132) == -1                                          # bf16 rows that do not start 16-byte aligned
    for fmt in (E4M3, E2M1):
        assert quant(rows=0, fmt=fmt) == 0
    assert quant(rows=0, x=None) == 0

    def score(ca=p, sa=p, cb=p, sb=p, ma=p, mb=p, wa=p, wb=p, out=p, NA=2, NB=3, T=4, Nv=5, D=128):
        return so.valor_fine_fused_fwd_mx(None, ca, sa, cb, sb, ma, mb, wa, wb, out, NA, NB, T, Nv, D)

    for name in ("ca", "sa", "cb", "sb", "ma", "mb", "wa", "wb", "out"):
        assert score(**{name: None}) == -1, name
    assert score(D=64) == -1 and score(D=0) == -1 and score(D=192) == -1 and score(D=32) == -1
    assert score(T=0) == -1 and score(T=65) == -1 and score(Nv=0) == -1 and score(Nv=65) == -1
    assert score(ca=p + 8) == -1 and score(cb=p + 8) == -1 and score(sa=p + 2) == -1 and score(sb=p + 1) == -1
    assert score(NA=1 << 20, T=64, D=128 * 512) == -1                   # past the byte limit of the buffer descriptor
    assert score(NA=-1) == -1 and score(NB=-1) == -1
    assert score(NA=0) == 0 and score(NB=0) == 0 and score(NA=0, ca=None) == 0


# ------------------------------------------------------------------ 3. the index on CPU tensors
def _cpu_mx_index(exact=None):
    from valor_amd.search import RetrievalIndex, mx_quantize_rows_host
    g = torch.Generator().manual_seed(1)
    feats = torch.randn((6, 10, 128), generator=g).bfloat16()
    weights = torch.softmax(torch.randn((6, 10), generator=g), dim=-1)
    codes, scales = mx_quantize_rows_host(feats, E2M1)
    return RetrievalIndex("tv", "fine", False, [codes], [weights], [f"c{j}" for j in range(6)], "mxfp4", scales=[scales], dtype=torch.bfloat16,
                          exact=exact, exact_feats=None if exact is None else [feats]), feats


@pytest.mark.parametrize("exact,tag", [(None, "/4"), ("device", "/5"), ("host", "/5")])
def test_mx_blob_round_trips(tmp_path, exact, tag):
    from valor_amd.search import RetrievalIndex
    index, feats = _cpu_mx_index(exact)
    assert index.bank_dtype == "mxfp4" and index.dtype == torch.bfloat16 and index.dim == 128
    assert index.feats[0].dtype == torch.uint8 and index.feats[0].shape == (6, 10, 64)
    assert index.scales[0].dtype == torch.uint8 and index.scales[0].shape == (6, 10, 4)
    want = {"group": "tv", "contra_type": "fine", "late_fusion": False, "D": 128, "tokens": [10], "dtype": "torch.bfloat16", "bank_dtype": "mxfp4_e2m1"}
    if exact is not None:
        want["exact"] = exact
    assert index.fingerprint() == want
    # codes, scale bytes and the fp32 token weights; a device store adds the bf16 features
    assert index.bank_bytes() == 6 * 10 * (64 + 4 + 4) + (6 * 10 * 128 * 2 if exact == "device" else 0)
    path = tmp_path / "bank_mx.pt"
    index.save(path)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert blob["format"] == "valor_amd.RetrievalIndex" + tag
    assert sorted(blob) == sorted(["codes", "fingerprint", "format", "ids", "scales", "weights"] + (["exact_feats"] if exact else []))
    back = RetrievalIndex.load(path, "cpu")
    assert back.bank_dtype == "mxfp4" and back.exact == exact and back.ids == index.ids and back.fingerprint() == index.fingerprint()
    for a, b in zip(back.feats + back.scales + back.weights + (back.exact_feats or []), index.feats + index.scales + index.weights + (index.exact_feats or [])):
        assert a.dtype == b.dtype and torch.equal(a, b)
    if exact:
        assert torch.equal(back.exact_feats[0], feats)


def test_load_refuses_a_format_4_blob_whose_fingerprint_disagrees(tmp_path):
    from valor_amd.search import RetrievalIndex
    index, _ = _cpu_mx_index()
    path = tmp_path / "bank_mx.pt"
    index.save(path)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    for key, value in (("D", 256), ("tokens", [8]), ("bank_dtype", "fp8_e4m3"), ("dtype", "torch.float16")):
        bad = dict(blob, fingerprint=dict(blob["fingerprint"], **{key: value}))
        torch.save(bad, path)
        with pytest.raises(ValueError):
            RetrievalIndex.load(path, "cpu")
    torch.save(dict(blob, format="valor_amd.RetrievalIndex/6"), path)
    with pytest.raises(ValueError, match="not a RetrievalIndex file"):
        RetrievalIndex.load(path, "cpu")
    # an fp8 blob is still an fp8 blob: the two code layouts are not confused
    torch.save(dict(blob, format="valor_amd.RetrievalIndex/2"), path)
    with pytest.raises(ValueError):
        RetrievalIndex.load(path, "cpu")


def test_what_an_mxfp4_bank_refuses():
    from valor_amd.search import RetrievalIndex, mx_quantize_rows_host
    pooled = torch.zeros((4, 128), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="mxfp4.*only fine banks"):
        RetrievalIndex.from_features(pooled, group="tv", contra_type="coarse", bank_dtype="mxfp4")
    with pytest.raises(ValueError, match="mxfp4.*only fine banks"):
        RetrievalIndex("tv", "coarse", False, [pooled], [None], list(range(4)), "mxfp4")
    with pytest.raises(ValueError, match="mxfp4.*only fine banks"):
        RetrievalIndex("tv", "coarse", False, [pooled], [None], list(range(4))).quantize(bank_dtype="mxfp4")
    w = lambda n: torch.full((4, n), 1.0 / n)
    with pytest.raises(ValueError, match="mxfp4.*D % 128"):             # no GEMM fallback for other geometries
        RetrievalIndex("tv", "fine", False, [torch.zeros((4, 10, 64), dtype=torch.bfloat16)], [w(10)], list(range(4)), "mxfp4")
    with pytest.raises(ValueError, match="mxfp4.*64 tokens"):
        RetrievalIndex("tv", "fine", False, [torch.zeros((4, 65, 128), dtype=torch.bfloat16)], [w(65)], list(range(4)), "mxfp4")
    for unknown in ("int8", "mxfp6", "fp4"):
        with pytest.raises(ValueError, match="bank_dtype"):
            RetrievalIndex("tv", "fine", False, [torch.zeros((4, 10, 128), dtype=torch.bfloat16)], [w(10)], list(range(4)), unknown)
    bf16 = RetrievalIndex("tv", "fine", False, [torch.zeros((4, 10, 128), dtype=torch.bfloat16)], [w(10)], list(range(4)))
    with pytest.raises(ValueError, match="bank_dtype"):
        bf16.quantize(bank_dtype="int8")
    # given as codes: the scale bytes must be uint8 [clips, tokens, D / 32]
    codes, scales = mx_quantize_rows_host(torch.randn((4, 10, 128)), E2M1)
    for bad in (scales.float(), scales[:, :, :2], scales[:, :5]):
        with pytest.raises(ValueError, match="mxfp4 bank given as codes"):
            RetrievalIndex("tv", "fine", False, [codes], [w(10)], list(range(4)), "mxfp4", scales=[bad], dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="mxfp4 bank given as codes"):
        RetrievalIndex("tv", "fine", False, [codes], [w(10)], list(range(4)), "mxfp4", scales=[scales], dtype=torch.float16)


def test_the_exact_store_rules_of_an_mxfp4_bank():
    from valor_amd.search import RetrievalIndex, mx_quantize_rows_host
    with pytest.raises(ValueError, match="exact"):
        _cpu_mx_index("disk")
    feats = torch.randn((4, 10, 128), generator=torch.Generator().manual_seed(2)).bfloat16()
    w = torch.full((4, 10), 0.1)
    codes, scales = mx_quantize_rows_host(feats, E2M1)
    make = lambda **kw: RetrievalIndex("tv", "fine", False, [codes], [w], list(range(4)), "mxfp4", scales=[scales], **kw)
    with pytest.raises(ValueError, match="bf16 features"):              # codes without the features they were made from
        make(dtype=torch.bfloat16, exact="device")
    with pytest.raises(ValueError, match="bf16 features"):              # an fp32 store: fp32 pair scores are not covered
        make(dtype=torch.float32, exact="device", exact_feats=[feats.float()])
    with pytest.raises(ValueError, match="bf16 features"):              # a store of another shape (the code rows' D / 2, say)
        make(dtype=torch.bfloat16, exact="host", exact_feats=[feats[:, :, :64].contiguous()])
    index = make(dtype=torch.bfloat16, exact="device", exact_feats=[feats])
    assert index.default_shortlist(5) == min(256, index.default_shortlist(1) * 5) and index.default_shortlist(100) == 256
    q = {"feat_t": torch.zeros((2, 6, 128), dtype=torch.bfloat16)}
    for k, shortlist in ((5, 4), (5, 257), (5, -1), (200, 100)):
        with pytest.raises(ValueError, match="shortlist"):
            index.search(None, q, k, shortlist=shortlist)
    with pytest.raises(ValueError, match="no shortlist"):
        index.search(None, q, 5, within=torch.zeros((2, 3), dtype=torch.int64), shortlist=20)
    plain = make(dtype=torch.bfloat16)
    cand = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="mxfp4 bank with an exact store"):
        plain.search(None, q, 5, shortlist=20)
    with pytest.raises(ValueError, match="mxfp4 bank keeps no exact store"):    # no fallback to the fp4 scores
        plain.rescore(None, q, cand)
    with pytest.raises(ValueError, match="exact store"):
        plain.search(None, q, 2, within=cand)
    with pytest.raises(ValueError, match="exact store"):
        plain.explain(None, q, cand)
    with pytest.raises(ValueError, match="exact store"):
        plain.search(None, q, 2, explain=True)
