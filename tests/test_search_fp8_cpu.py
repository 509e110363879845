"""The fp8 clip bank without a GPU: the quantisation law on hand-made rows (expected bytes written out), the score law against the
project's oracle on the dequantised rows, argument validation of the two entry points, and the persistence / refusal rules on CPU tensors."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# (row, expected codes, expected scale): the hand-made rows, shared with tests/test_search_fp8_gpu.py (padded there to 16 columns)
S = 2.0 ** -9                                                          # the smallest e4m3 subnormal
HAND_ROWS = [
    # a zero row, and an amax below 2^-64: scale 0, codes 0
    ([0.0, -0.0, 0.0, 0.0], [0x00, 0x00, 0x00, 0x00], 0.0),
    ([2.0 ** -65, -2.0 ** -66, 0.0, 0.0], [0x00, 0x00, 0x00, 0x00], 0.0),
    # the amax element is negative: -448 = 0xFE; 1 * inv = 149.33 -> 144 = 0x71, 0.5 * inv = 74.67 -> 72 = 0x69
    ([-3.0, 1.0, 0.5, 0.0], [0xFE, 0x71, 0x69, 0x00], float.fromhex("0x1.b6db6ep-8")),
    # one outlier (inv == 1) puts the rest into the subnormal range (steps of 2^-9): exact values, ties to even (2^-10 -> 0, 1.5 -> 2,
    # 2.5 -> 2), the sign kept on a value that rounds to zero, 2^-6 the smallest normal
    ([448.0, S, 3 * S, S / 2, 1.5 * S, -S, 8 * S, -S / 2, 2.5 * S, S / 4], [0x7E, 0x01, 0x03, 0x00, 0x02, 0x81, 0x08, 0x80, 0x02, 0x00], 1.0),
    # inv == 1 and y exactly on ties of the binade [16, 32) (steps of 2): 17 -> 16, 19 -> 20, 21 -> 20, 23 -> 24
    ([448.0, 17.0, 19.0, 21.0, 23.0, -17.0, -19.0, 0.0], [0x7E, 0x58, 0x5A, 0x5A, 0x5C, 0xD8, 0xDA, 0x00], 1.0),
    # fl(amax * fl(448 / amax)) = 448.00003 > 448: the clamp gives 0x7E / 0xFE, never NaN (0x7F)
    ([float.fromhex("0x1.8ac7fep+1"), -float.fromhex("0x1.8ac7fep+1"), float.fromhex("0x1.8ac7fep+0"), 0.0], [0x7E, 0xFE, 0x76, 0x00],
     float.fromhex("0x1.c32db4p-8")),
]


def test_quantize_rows_host_on_hand_made_rows():
    from valor_amd.search import quantize_rows_host
    for row, want_codes, want_scale in HAND_ROWS:
        x = torch.tensor([row], dtype=torch.float32)
        codes, scale = quantize_rows_host(x)
        assert codes.dtype == torch.uint8 and scale.dtype == torch.float32 and codes.shape == x.shape and scale.shape == (1,)
        assert codes[0].tolist() == want_codes, (row, [hex(c) for c in codes[0].tolist()])
        assert scale.item() == want_scale, (row, scale.item().hex())
    x = torch.tensor([float.fromhex("0x1.8ac7fep+1")])
    assert float(x * (torch.full_like(x, 448.0) / x)) > 448.0           # the last row does leave the range before the clamp
    # leading dimensions are kept, bf16 input is widened exactly
    x = torch.randn((3, 5, 32), generator=torch.Generator().manual_seed(0)).bfloat16()
    c3, s3 = quantize_rows_host(x)
    c2, s2 = quantize_rows_host(x.float().view(15, 32))
    assert c3.shape == (3, 5, 32) and s3.shape == (3, 5) and torch.equal(c3.view(15, 32), c2) and torch.equal(s3.view(15), s2)
    assert not bool((c3 & 0x7F == 0x7F).any())


def test_fp8_scores_host_against_the_oracle_on_dequantised_rows():
    """Oracle.compute_fine_matrix in fp32 on code * scale, band 2e-5 + 1e-5 |s|: the new score law is the project's"""
    import valor_oracle as VO
    from valor_amd.search import fp8_scores_host, quantize_rows_host
    NA, NB, T, Nv, D = 5, 9, 7, 10, 128
    g = torch.Generator().manual_seed(3)
    fa, fb = torch.randn((NA, T, D), generator=g), torch.randn((NB, Nv, D), generator=g)
    ca, sa = quantize_rows_host(fa)
    cb, sb = quantize_rows_host(fb)
    maskA = (torch.arange(T)[None] < torch.tensor([7, 1, 4, 6, 2])[:, None]).long()
    maskB = torch.ones((NB, Nv), dtype=torch.long)
    maskB[2, 7:] = 0
    rawA, rawB = torch.randn((NA, T), generator=g), torch.randn((NB, Nv), generator=g)
    deq = lambda c, s: c.view(torch.float8_e4m3fn).float() * s[..., None]
    want = VO.Oracle.compute_fine_matrix(deq(ca, sa), deq(cb, sb), maskA, maskB, rawA, rawB)
    soft = lambda raw, m: torch.softmax(raw.masked_fill(m == 0, float("-inf")), dim=-1)
    got = fp8_scores_host(ca, sa, cb, sb, maskA, maskB, soft(rawA, maskA), soft(rawB, maskB))
    assert got.dtype == torch.float64 and got.shape == (NA, NB)
    err = (got - want.double()).abs()
    print(f"largest |fp8_scores_host - oracle| {float(err.max()):.3g}")
    assert bool((err <= 2e-5 + 1e-5 * want.double().abs()).all())


def test_argument_validation_without_gpu():
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0

    def quant(x=p, ld=128, rows=4, cols=128, codes=p, scales=p, dtype=0):
        return so.valor_fp8_quantize_rows(None, dtype, x, ld, rows, cols, codes, scales)

    assert quant(x=None) == -1 and quant(codes=None) == -1 and quant(scales=None) == -1
    assert quant(cols=8) == -1 and quant(cols=0) == -1 and quant(cols=24) == -1
    assert quant(ld=64) == -1 and quant(dtype=7) == -1 and quant(x=p + 2) == -1 and quant(codes=p + 4) == -1
    assert quant(rows=0) == 0 and quant(rows=0, x=None) == 0

    def score(ca=p, sa=p, cb=p, sb=p, ma=p, mb=p, wa=p, wb=p, out=p, NA=2, NB=3, T=4, Nv=5, D=128):
        return so.valor_fine_fused_fwd_fp8(None, ca, sa, cb, sb, ma, mb, wa, wb, out, NA, NB, T, Nv, D)

    for name in ("ca", "sa", "cb", "sb", "ma", "mb", "wa", "wb", "out"):
        assert score(**{name: None}) == -1, name
    assert score(D=64) == -1 and score(D=0) == -1 and score(D=192) == -1
    assert score(T=0) == -1 and score(T=65) == -1 and score(Nv=0) == -1 and score(Nv=65) == -1
    assert score(ca=p + 8) == -1 and score(cb=p + 8) == -1
    assert score(NA=1 << 20, T=64, D=128 * 512) == -1                   # past the byte limit of the buffer descriptor
    assert score(NA=0) == 0 and score(NB=0) == 0 and score(NA=0, ca=None) == 0


def _cpu_fine_index(bank_dtype=None):
    from valor_amd.search import RetrievalIndex, quantize_rows_host
    g = torch.Generator().manual_seed(1)
    feats = torch.randn((6, 10, 128), generator=g).bfloat16()
    weights = torch.softmax(torch.randn((6, 10), generator=g), dim=-1)
    ids = [f"c{j}" for j in range(6)]
    if bank_dtype is None:
        return RetrievalIndex("tv", "fine", False, [feats], [weights], ids)
    codes, scales = quantize_rows_host(feats)
    return RetrievalIndex("tv", "fine", False, [codes], [weights], ids, "fp8", scales=[scales], dtype=torch.bfloat16)


def test_unquantised_index_describes_and_saves_as_before(tmp_path):
    index = _cpu_fine_index()
    assert index.bank_dtype is None and index.scales is None
    assert index.fingerprint() == {"group": "tv", "contra_type": "fine", "late_fusion": False, "D": 128, "tokens": [10], "dtype": "torch.bfloat16"}
    index.save(tmp_path / "bank.pt")
    blob = torch.load(tmp_path / "bank.pt", map_location="cpu", weights_only=True)
    assert blob["format"] == "valor_amd.RetrievalIndex/1" and sorted(blob) == ["feats", "fingerprint", "format", "ids", "weights"]
    assert index.bank_bytes() == 6 * 10 * 128 * 2 + 6 * 10 * 4


def test_fp8_blob_round_trips(tmp_path):
    from valor_amd.search import RetrievalIndex
    index = _cpu_fine_index("fp8")
    assert index.bank_dtype == "fp8" and index.dtype == torch.bfloat16 and index.feats[0].dtype == torch.uint8
    assert index.fingerprint() == {"group": "tv", "contra_type": "fine", "late_fusion": False, "D": 128, "tokens": [10], "dtype": "torch.bfloat16",
                                   "bank_dtype": "fp8_e4m3"}
    assert index.bank_bytes() == 6 * 10 * 128 + 2 * 6 * 10 * 4
    index.save(tmp_path / "bank8.pt")
    blob = torch.load(tmp_path / "bank8.pt", map_location="cpu", weights_only=True)
    assert blob["format"] == "valor_amd.RetrievalIndex/2" and blob["codes"][0].dtype == torch.uint8
    back = RetrievalIndex.load(tmp_path / "bank8.pt", "cpu")
    assert back.bank_dtype == "fp8" and back.dtype == torch.bfloat16 and back.ids == index.ids and back.fingerprint() == index.fingerprint()
    for a, b in zip(back.feats + back.scales + back.weights, index.feats + index.scales + index.weights):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_what_an_fp8_bank_refuses():
    from valor_amd.search import RetrievalIndex
    pooled = torch.zeros((4, 128), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="only fine banks"):
        RetrievalIndex.from_features(pooled, group="tv", contra_type="coarse", bank_dtype="fp8")
    with pytest.raises(ValueError, match="only fine banks"):
        RetrievalIndex("tv", "coarse", False, [pooled], [None], list(range(4)), "fp8")
    with pytest.raises(ValueError, match="only fine banks"):
        RetrievalIndex("tv", "coarse", False, [pooled], [None], list(range(4))).quantize()
    w = lambda n: torch.full((4, n), 1.0 / n)
    with pytest.raises(ValueError, match="D % 128"):                    # no GEMM fallback for other geometries
        RetrievalIndex("tv", "fine", False, [torch.zeros((4, 10, 64), dtype=torch.bfloat16)], [w(10)], list(range(4)), "fp8")
    with pytest.raises(ValueError, match="64 tokens"):
        RetrievalIndex("tv", "fine", False, [torch.zeros((4, 65, 128), dtype=torch.bfloat16)], [w(65)], list(range(4)), "fp8")
    with pytest.raises(ValueError, match="bank_dtype"):
        RetrievalIndex("tv", "fine", False, [torch.zeros((4, 10, 128), dtype=torch.bfloat16)], [w(10)], list(range(4)), "int8")
