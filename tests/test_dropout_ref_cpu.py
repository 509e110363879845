"""The host restatement of the dropout mask laws (tests/dropout_ref.py): the vectorised numpy functions against a scalar transcription in
Python ints, the LayerNorm mask against the Philox words it is built from, and the quality of the attention hash at the model's setting
(p = 0.1) measured ON THE RESTATEMENT -- the GPU tests pin every kernel family to it bit for bit
(tests/test_attention_dropout_gpu.py, tests/test_layernorm_dropout_gpu.py)."""
import math
import random

import numpy as np
import pytest

import dropout_ref as R


def _rand_seed_offset(rng, i):
    seed = rng.getrandbits(64) if i % 2 else rng.getrandbits(31)
    if i % 3 == 0:
        seed |= 1 << (32 + rng.randrange(32))                 # seed >= 2^32: the high word enters the head key
    offset = rng.getrandbits(64) if i % 4 == 0 else rng.getrandbits(20)
    if i % 5 == 0:
        offset = (3 << 40) + 12345 + rng.getrandbits(24)      # offset >= 2^40: a device-mode step's base
    if i == 7:
        offset = (1 << 64) - 3                                # by-value offset + base wraps modulo 2^64
    return seed, offset


def test_vectorised_attention_hash_equals_the_scalar_transcription():
    rng = random.Random(1)
    n = big_seed = big_offset = 0
    for i in range(48):
        seed, offset = _rand_seed_offset(rng, i)
        big_seed += seed >= 1 << 32
        big_offset += offset >= 1 << 40
        heads = [rng.randrange(0, 1 << 12) for _ in range(80)] + [0, 1, (1 << 31) - 1]
        idx = [rng.randrange(0, 1 << 24) for _ in range(80)] + [0, (1 << 24) - 1, 1 << 23]
        hk = R.attn_drop_headkey(seed, offset, np.array(heads))
        bits = R.attn_drop_bits(hk, np.array(idx, dtype=np.uint64))
        for h, e, k_, b_ in zip(heads, idx, hk, bits):
            ks = R.attn_drop_headkey_scalar(seed, offset, h)
            assert int(k_) == ks and 0 <= ks <= R.M32
            assert int(b_) == R.attn_drop_bits_scalar(ks, e)
            n += 1
    assert n >= 3000 and big_seed >= 10 and big_offset >= 10
    xs = [rng.getrandbits(32) for _ in range(500)] + [0, R.M32]
    assert [int(v) for v in R.mix32(np.array(xs, dtype=np.uint64))] == [R.mix32_scalar(x) for x in xs]


def test_umul24_uses_the_low_24_bits_only():
    """bits 24-31 of (index ^ hk) do not reach the first product, and a product beyond 2^32 keeps its low word"""
    hk = 0xDEADBEEF
    want = R.attn_drop_bits_scalar(hk, 5)
    x = (5 ^ hk) & 0xFFFFFF
    y = (x * 0x9E3779 + (hk >> 7)) & R.M32
    y ^= y >> 15
    y = ((y & 0xFFFFFF) * 0x85EBCB + hk) & R.M32
    assert want == y ^ (y >> 13)
    assert x * 0x9E3779 > R.M32                                # the case exercises the truncation


def test_drop_threshold_takes_p_as_float32():
    assert R.drop_threshold(0.0) == 0 and R.drop_threshold(0.5) == 1 << 31 and R.drop_threshold(0.25) == 1 << 30
    assert R.drop_threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32) == 429496736     # not int(0.1 * 2^32) = 429496729
    assert R.drop_threshold(0.99999999) == 0xFFFFFFFF


def test_attn_keep_layout():
    """[B, H, Sq, Skv]: head index b * H + h, element index q * Skv + j with the pitch Skv whatever kv_range says"""
    B, H, Sq, Skv, p = 3, 2, 5, 70, 0.1
    seed, offset = (9 << 32) + 7, (3 << 40) + 12345 + 11
    kvr = np.array([[0, 70], [0, 20], [20, 50]])
    keep = R.attn_keep(seed, offset, B, H, Sq, Skv, p, kv_range=kvr)
    assert keep.shape == (B, H, Sq, Skv) and keep.dtype == np.bool_
    assert np.array_equal(keep, R.attn_keep(seed, offset, B, H, Sq, Skv, p))
    thr = R.drop_threshold(p)
    rng = random.Random(2)
    for _ in range(600):
        b, h, q, j = rng.randrange(B), rng.randrange(H), rng.randrange(Sq), rng.randrange(Skv)
        hk = R.attn_drop_headkey_scalar(seed, offset, b * H + h)
        assert bool(keep[b, h, q, j]) == (R.attn_drop_bits_scalar(hk, q * Skv + j) >= thr)
    sel = R.attn_keep_heads(seed, offset, [4, 1], Sq, Skv, p)
    assert np.array_equal(sel[0], keep[2, 0]) and np.array_equal(sel[1], keep[0, 1])


def test_ln_keep_equals_the_philox_words():
    rng = random.Random(3)
    for rows, cols, seed, offset, p in ((37, 100, 7, 11, 0.1), (9, 768, (5 << 32) + 1, (3 << 40) + 12345 + 77, 0.25), (4, 2052, 1234, (1 << 64) - 2, 0.1)):
        keep = R.ln_keep(seed, offset, rows, cols, p)
        assert keep.shape == (rows, cols) and keep.dtype == np.bool_
        thr = R.drop_threshold(p)
        words = R.philox4x32_10(seed, np.uint64(offset) + np.arange(rows * cols // 4, dtype=np.uint64))       # the masker test's Philox
        flat = keep.reshape(-1)
        for w in range(4):
            assert np.array_equal(flat[w::4], words[w] >= np.uint64(thr))
        for _ in range(300):
            r, c = rng.randrange(rows), rng.randrange(cols)
            ctr = (offset + (r * cols + c) // 4) & R.M64
            assert bool(keep[r, c]) == (R.philox4x32_10_scalar(seed, ctr)[c % 4] >= thr)


def test_vectorised_philox_equals_the_scalar_transcription():
    rng = random.Random(4)
    for i in range(20):
        seed, offset = _rand_seed_offset(rng, i)
        ctrs = [(offset + rng.getrandbits(30)) & R.M64 for _ in range(50)]
        got = R.philox4x32_10(seed, np.array(ctrs, dtype=np.uint64))
        for j, c in enumerate(ctrs):
            assert tuple(int(w[j]) for w in got) == R.philox4x32_10_scalar(seed, c)


# ---------------------------------------------------------------------------------------------- mask quality at the model's setting
P, SEED, OFFSET = 0.1, 7, 11
SHAPES = [(24, 197, 197), (24, 129, 129), (48, 32, 32), (24, 42, 1834)]      # (B * H, Sq, Skv): ViT frame, AST slice, text, decoder cross-attention


def _kprob(p):
    return 1.0 - R.drop_threshold(p) / 2.0 ** 32


def _corr_sigmas(a, b, k):
    """sum of (a - k)(b - k) over the pairs in units of its standard deviation under independence, sqrt(N) k (1 - k)"""
    a, b = a.astype(np.float64).reshape(-1) - k, b.astype(np.float64).reshape(-1) - k
    return float((a * b).sum() / (math.sqrt(a.size) * k * (1.0 - k)))


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_mask_quality(shape):
    """keep fraction and the correlation of keep bits with the neighbouring key, query row, head, seed and with the next window as
    DropoutState.draw_elems lays it out: each within 5 sigma of independent Bernoulli(1 - p) draws."""
    BH, Sq, Skv = shape
    k = _kprob(P)
    heads = np.arange(BH)
    m = R.attn_keep_heads(SEED, OFFSET, heads, Sq, Skv, P)
    stats = {"fraction": (m.mean() - k) / math.sqrt(k * (1 - k) / m.size),
             "key/key+1": _corr_sigmas(m[:, :, :-1], m[:, :, 1:], k),
             "q/q+1": _corr_sigmas(m[:, :-1], m[:, 1:], k),
             "head/head+1": _corr_sigmas(m[:-1], m[1:], k),
             "seed/seed+1": _corr_sigmas(m, R.attn_keep_heads(SEED + 1, OFFSET, heads, Sq, Skv, P), k),
             "next window": _corr_sigmas(m, R.attn_keep_heads(SEED, OFFSET + BH * Sq * Skv + 1, heads, Sq, Skv, P), k)}
    print(shape, {n: round(float(v), 2) for n, v in stats.items()})
    for n, v in stats.items():
        assert abs(v) < 5.0, (shape, n, v)


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_mask_per_row_spread(shape):
    """the standard deviation of the per-row keep fraction against the binomial one, sqrt(k (1 - k) / Skv). The two-round 24-bit hash
    spreads the drops of a row slightly MORE evenly than independent draws would (observed: about 3.5 % under binomial at p = 0.1 and
    9 % under at p = 0.5): asserted within +-10 % at p = 0.1."""
    BH, Sq, Skv = shape
    k = _kprob(P)
    m = R.attn_keep_heads(SEED, OFFSET, np.arange(BH), Sq, Skv, P)
    ratio = m.mean(axis=2).std() / math.sqrt(k * (1 - k) / Skv)
    print(shape, "per-row spread / binomial", round(float(ratio), 4))
    assert abs(ratio - 1.0) < 0.10, (shape, ratio)


def test_layernorm_mask_keep_fraction():
    rows, cols = 333, 768
    k = _kprob(P)
    m = R.ln_keep(SEED, OFFSET, rows, cols, P)
    z = (m.mean() - k) / math.sqrt(k * (1 - k) / m.size)
    print("ln_keep fraction", float(m.mean()), "sigmas", round(float(z), 2))
    assert abs(z) < 5.0, z
