"""Caption sampling filters without a GPU: the library exports valor_sample_tokens_filtered and validates its arguments before any launch;
the Sampling value type; generate_cap's argument errors; the host restatement of the top-k / top-p rules (decode.filter_row) on
hand-made rows with known answers and on the two rows the GPU tests use."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import decode, synth                    # noqa: E402
from valor_amd.model.valor import VALOR                 # noqa: E402

INF = float("inf")


def test_library_exports_the_symbol_and_the_binding_knows_it():
    from valor_amd import lib
    so = lib.load()
    assert hasattr(so, "valor_sample_tokens_filtered")
    assert len(lib.SIGNATURES["valor_sample_tokens_filtered"]) == 19


def test_filtered_sampler_validates_arguments_without_gpu():
    from valor_amd import lib
    so = lib.load()
    f = (ctypes.c_float * 64)()
    u8 = (ctypes.c_uint8 * 4)()
    i64 = (ctypes.c_int64 * 16)()
    i32 = (ctypes.c_int32 * 4)()

    def call(R=4, V=16, ld=16, eos=3, inv=1.0, k=0, p=0.9, logits=f, unf=u8, tok=i64, sents=i64, sents_ld=1, lp=f, lp_ld=1):
        return so.valor_sample_tokens_filtered(None, logits, ld, R, V, 1, 0, eos, inv, k, p, unf, tok, sents, sents_ld, lp, lp_ld, i32, f)
    assert call(R=0) == 0                                                         # no rows: no-op, nothing is checked or launched
    assert call(R=0, logits=None) == 0
    assert call(R=-1) == -1 and call(V=0) == -1 and call(ld=8) == -1
    assert call(eos=16) == -1 and call(eos=-1) == -1
    for bad in (0.0, -1.0, INF, float("nan")):
        assert call(inv=bad) == -1, bad
    for bad in (0.0, -0.5, 1.0000001, float("nan"), INF):
        assert call(p=bad) == -1, bad
    assert call(k=-1) == -1
    assert call(sents_ld=-1) == -1 and call(lp_ld=-1) == -1
    assert call(logits=None) == -1 and call(unf=None) == -1 and call(tok=None) == -1 and call(sents=None) == -1 and call(lp=None) == -1


def test_sampling_validates_its_fields():
    s = decode.Sampling()
    assert s.off and (s.temperature, s.top_k, s.top_p) == (1.0, 0, 1.0) and s.inv_temperature == 1.0
    s = decode.Sampling(temperature=0.7, top_k=50, top_p=0.9)
    assert not s.off and s.top_k == 50
    assert s.inv_temperature == float(torch.tensor(1 / 0.7, dtype=torch.float32))
    assert not decode.Sampling(top_k=1).off and not decode.Sampling(top_p=0.5).off and not decode.Sampling(temperature=2).off
    with pytest.raises(ValueError, match="greedy"):
        decode.Sampling(temperature=0)
    for t in (-1.0, INF, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            decode.Sampling(temperature=t)
    for k in (-1, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            decode.Sampling(top_k=k)
    for p in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            decode.Sampling(top_p=p)


def test_generate_cap_argument_errors():
    m = VALOR(None, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu")
    for kw in ({"temperature": 0.7}, {"top_k": 5}, {"top_p": 0.9}, {"num_return_sequences": 2}):
        for mode in (None, "greedy"):
            with pytest.raises(ValueError, match="mode='sample'"):
                decode.generate_cap(m, {}, ["tv"], mode=mode, **kw)
    with pytest.raises(ValueError, match="greedy"):
        decode.generate_cap(m, {}, ["tv"], mode="sample", temperature=0)
    with pytest.raises(ValueError, match="top_p"):
        decode.generate_cap(m, {}, ["tv"], mode="sample", top_p=0.0)
    with pytest.raises(ValueError, match="top_k"):
        decode.generate_cap(m, {}, ["tv"], mode="sample", top_k=-3)
    for n in (0, -1, 1.5):
        with pytest.raises(ValueError, match="num_return_sequences"):
            decode.generate_cap(m, {}, ["tv"], mode="sample", num_return_sequences=n)
    bad = VALOR({"sample_top_p": 2.0}, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError, match="top_p"):                              # the model's options go through the same validation
        decode.generate_cap(bad, {}, ["tv"], mode="sample")


def test_sampling_signatures_keep_their_defaults():
    import inspect
    assert inspect.signature(decode.decode_sample).parameters["sampling"].default is None
    p = inspect.signature(decode.generate_cap).parameters
    assert p["temperature"].default is None and p["top_k"].default is None and p["top_p"].default is None
    assert p["num_return_sequences"].default == 1


def test_filter_row_hand_made_rows():
    F = decode.filter_row
    y = torch.tensor([1.0, 3.0, 2.0, 3.0, 0.0, 2.0])
    assert F(y) == (6, 0.0)
    assert F(y, top_k=1) == (2, 3.0)                      # duplicates at the k-th value: kept > top_k
    assert F(y, top_k=2) == (2, 3.0)
    assert F(y, top_k=3) == (4, 2.0)
    assert F(y, top_k=5) == (5, 1.0)
    assert F(y, top_k=6) == (6, 0.0) and F(y, top_k=13) == (6, 0.0)            # top_k at / above the finite count: off
    z = torch.tensor([-INF, 2.0, -INF, 1.0, 0.5, -INF])
    assert F(z) == (3, 0.5)                               # -inf columns are never kept
    assert F(z, top_k=3) == (3, 0.5) and F(z, top_k=5) == (3, 0.5)             # top_k above the finite count
    assert F(z, top_k=2) == (2, 1.0)
    assert F(torch.full((4,), -INF), top_k=2, top_p=0.5)[0] == 0 and math.isnan(F(torch.full((4,), -INF))[1])
    # top-p: masses 1/2, 1/4, 1/8, 1/8 (log 4, log 2, 0, 0)
    q = torch.tensor([0.0, math.log(4.0), math.log(2.0), 0.0], dtype=torch.float64)
    assert F(q, top_p=0.4) == (1, math.log(4.0))
    assert F(q, top_p=0.6) == (2, math.log(2.0))
    assert F(q, top_p=0.8) == (4, 0.0)                    # the running mass reaches 0.8 inside the tie: both tied columns stay
    assert F(q, top_p=1.0) == (4, 0.0)
    assert F(q, top_p=1e-9) == (1, math.log(4.0))         # never empty: the arg max stays
    # top-p over what top-k left: S_k = the three largest (masses 4, 2, 1 of 7); 0.6 * 7 = 4.2 -> two columns
    q2 = torch.tensor([0.0, math.log(4.0), math.log(2.0), -1.0], dtype=torch.float64)
    assert F(q2, top_k=3, top_p=0.6) == (2, math.log(2.0))
    assert F(q2, top_k=1, top_p=0.6) == (1, math.log(4.0))


def dominant_row():
    """the row of tests/test_scst_gpu.py::test_sampler_law_vocab_dominant, fp32"""
    g = torch.Generator().manual_seed(3)
    row = torch.randn(30522, generator=g, dtype=torch.float64) * 0.5
    row[[17, 4000, 30000]] = torch.tensor([9.0, 8.5, 8.0], dtype=torch.float64)
    return row.float()


def flat_row(V=30522):
    return (torch.randn(V, generator=torch.Generator().manual_seed(11)) * 2).float()


INV07 = float(torch.tensor(1 / 0.7, dtype=torch.float32))
DOMINANT_CASES = ((1.0, 0.3, 3), (INV07, 0.3, 1), (INV07, 0.6, 2), (INV07, 0.8, 2), (INV07, 0.9, 3))
FLAT_CASES = ((1.0, 0.5, 766), (1.0, 0.9, 7368), (INV07, 0.5, 110), (INV07, 0.9, 2047))


def test_filter_row_reproduces_the_nucleus_sizes_of_the_gpu_cases():
    row = dominant_row()
    for inv, p, want in DOMINANT_CASES:
        y = row * torch.tensor(inv, dtype=torch.float32)
        assert decode.filter_row(y, top_p=p)[0] == want, (inv, p)
    row = flat_row()
    for inv, p, want in FLAT_CASES:
        y = row * torch.tensor(inv, dtype=torch.float32)
        n = decode.filter_row(y, top_p=p)[0]
        lo, hi = decode.filter_row(y, top_p=p - 1e-4)[0], decode.filter_row(y, top_p=p + 1e-4)[0]
        assert n == want and lo <= n <= hi and hi - n <= 6 and n - lo <= 6, (inv, p, n, lo, hi)
