"""CPU: the host half of the device token masker (valor_amd/model/valor.py DeviceTokenMasker) -- the per-row count draw against the
exact law of Binomial(m, p) | k >= 1, the token_masker option / VALOR_MASKER switch, and argument validation of the two masker entry
points before they touch a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import synth  # noqa: E402
from valor_amd.model.valor import VALOR, DeviceTokenMasker, draw_mask_counts, token_masker_mode  # noqa: E402


def _truncated_binomial_pmf(m, p):
    """P(k) for k = 1..m of Binomial(m, p) conditioned on k >= 1, exact in float64"""
    from math import comb
    pmf = np.array([comb(m, k) * p ** k * (1 - p) ** (m - k) for k in range(1, m + 1)])
    return pmf / (1.0 - (1.0 - p) ** m)


@pytest.mark.parametrize("m", [1, 5, 30])
@pytest.mark.parametrize("p", [0.15, 0.6, 0.99])
def test_count_draw_matches_the_truncated_binomial(m, p):
    """chi-square of 40000 rows (fixed seed) against the exact pmf, bins with an expected count below 5 merged into their neighbour;
    the statistic stays within 6 sigma of its mean (normal approximation of chi2 with df degrees of freedom)"""
    N = 40000
    k = draw_mask_counts(np.full(N, m), p, np.random.default_rng(1234 + m))
    assert k.min() >= 1 and k.max() <= m
    if m == 1:
        assert (k == 1).all()
        return
    exp = _truncated_binomial_pmf(m, p) * N
    obs = np.bincount(k - 1, minlength=m).astype(np.float64)
    # merge sparse bins (tails) into the next one towards the mode
    e_b, o_b, e_acc, o_acc = [], [], 0.0, 0.0
    for e, o in zip(exp, obs):
        e_acc, o_acc = e_acc + e, o_acc + o
        if e_acc >= 5:
            e_b.append(e_acc); o_b.append(o_acc); e_acc = o_acc = 0.0
    if e_acc > 0:
        if e_b:
            e_b[-1] += e_acc; o_b[-1] += o_acc
        else:
            e_b.append(e_acc); o_b.append(o_acc)
    e_b, o_b = np.array(e_b), np.array(o_b)
    if len(e_b) == 1:                   # p = 0.99: essentially every row draws k = m
        assert o_b[0] == N
        return
    chi2 = float(((o_b - e_b) ** 2 / e_b).sum())
    df = len(e_b) - 1
    assert chi2 < df + 6 * np.sqrt(2 * df), (m, p, chi2, df)


def test_count_draw_redraws_only_zero_rows():
    """rows are independent: a row's draw does not depend on how many other rows needed a redraw (same generator state -> the rows
    that drew >= 1 the first time keep that value)"""
    m = np.array([1, 1, 1, 40, 40, 40, 2, 3])
    a = draw_mask_counts(m, 0.15, np.random.default_rng(7))
    first = np.random.default_rng(7).binomial(m, 0.15)
    keep = first > 0
    assert (a[keep] == first[keep]).all() and (a >= 1).all()


def test_token_masker_option(monkeypatch):
    monkeypatch.delenv("VALOR_MASKER", raising=False)
    assert token_masker_mode(None) == "host" and token_masker_mode({}) == "host"
    assert token_masker_mode({"token_masker": "device"}) == "device"
    monkeypatch.setenv("VALOR_MASKER", "device")
    assert token_masker_mode(None) == "device"
    monkeypatch.setenv("VALOR_MASKER", "host")
    assert token_masker_mode({"token_masker": "device"}) == "host"
    for bad in ("gpu", "Device", "hip"):
        monkeypatch.setenv("VALOR_MASKER", bad)
        with pytest.raises(ValueError, match="VALOR_MASKER"):
            token_masker_mode(None)
    monkeypatch.delenv("VALOR_MASKER")
    with pytest.raises(ValueError):
        token_masker_mode({"token_masker": "cuda"})


def test_model_reads_the_option_at_construction(monkeypatch):
    monkeypatch.delenv("VALOR_MASKER", raising=False)
    spec = synth.tiny_spec()
    m = VALOR(None, spec=spec, dtype=torch.float32, device="cpu")
    assert m.token_masker == "host" and m.device_masker is None
    monkeypatch.setenv("VALOR_MASKER", "device")
    m = VALOR({"seed": 9}, spec=spec, dtype=torch.float32, device="cpu")
    assert m.token_masker == "device" and isinstance(m.device_masker, DeviceTokenMasker)
    assert (m.device_masker.seed, m.device_masker.calls, m.device_masker.offset) == (9, 0, 0)
    assert m.device_masker.range == [106, spec.vocab] and m.device_masker.mask_token == m.text_mask_token
    monkeypatch.setenv("VALOR_MASKER", "both")
    with pytest.raises(ValueError):
        VALOR(None, spec=spec, dtype=torch.float32, device="cpu")


def test_device_masker_refuses_a_row_without_candidates():
    """as TokenMasker: a row whose only token is [CLS] (or all padding) is an error, raised before anything is uploaded"""
    mk = DeviceTokenMasker(103, 106, 1200, put=lambda t: pytest.fail("uploaded"), seed=1)
    toks = torch.tensor([[101, 2000, 102, 0], [101, 0, 0, 0]])
    with pytest.raises(ValueError):
        mk(toks, 0.15)
    assert mk.calls == 0 and mk.offset == 0


def test_philox_key_depends_on_seed_and_rank():
    a, b = DeviceTokenMasker(103, 106, 1200, None, seed=1), DeviceTokenMasker(103, 106, 1200, None, seed=2)
    keys = {a.philox_key(0), a.philox_key(1), b.philox_key(0), b.philox_key(1)}
    assert len(keys) == 4 and a.philox_key(1) == DeviceTokenMasker(103, 106, 1200, None, seed=1).philox_key(1)
    assert all(0 <= k < 1 << 64 for k in keys)


def test_masker_entries_validate_arguments_without_gpu():
    """valor_mask_tokens / valor_masked_rows return -1 on a bad argument before any launch; n = 0 rows is a no-op"""
    from valor_amd import lib
    so = lib.load()
    tok = (ctypes.c_int64 * 64)()
    k = (ctypes.c_int32 * 8)()
    out = (ctypes.c_int64 * 64)()

    def mask(tokens=tok, kk=k, b=2, T=32, rs=106, re=30522, o=out, lab=out):
        return so.valor_mask_tokens(None, tokens, kk, b, T, 1, 0, 103, rs, re, o, lab)

    assert mask(tokens=None) == -1 and mask(kk=None) == -1 and mask(o=None) == -1 and mask(lab=None) == -1
    assert mask(T=513) == -1 and mask(T=0) == -1
    assert mask(b=0) == -1 and mask(b=-3) == -1
    assert mask(rs=106, re=106) == -1 and mask(rs=200, re=106) == -1 and mask(rs=-1, re=10) == -1

    def rows(labels=tok, off=k, b=2, T=32, G=1, Ttot=32, r0=0, n=4, idx=out, lab=out):
        return so.valor_masked_rows(None, labels, off, b, T, G, Ttot, r0, n, idx, lab)

    assert rows(labels=None) == -1 and rows(off=None) == -1 and rows(idx=None) == -1 and rows(lab=None) == -1
    assert rows(T=513, Ttot=600) == -1 and rows(b=0) == -1 and rows(G=0) == -1 and rows(G=-1) == -1
    assert rows(Ttot=31) == -1 and rows(n=-1) == -1 and rows(r0=-5) == -1
    assert rows(n=0) == 0
