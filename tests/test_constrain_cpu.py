"""Generation controls without a GPU: the host law (decode.constrain_rows_host) against a deliberately naive per-row restatement on
random rows and on the hand-made histories the GPU kernel test uses; the Constraints value type; valor_logits_constrain's argument
validation before any launch; generate_cap / generate_qa argument errors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import decode, synth                    # noqa: E402
from valor_amd.model.valor import VALOR                 # noqa: E402

INF = float("inf")
# values a logit can hold: zeros of both signs, -inf, large and small magnitudes (1e-41 is subnormal; 3e38 / 0.5 overflows to inf)
SPECIAL = [0.0, -0.0, -INF, 1e30, -1e30, 1e-30, -1e-30, 1e-41, -1e-41, 3e38, -3e38, 2.5, -2.5]


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def naive_rows(logits, hist, t, penalty, n, min_len, suppress, eos, active=None):
    """the law, one position at a time: a set for the distinct tokens, tuples for the n-grams, numpy fp32 scalars for the multiply"""
    out = logits.clone()
    R, V = out.shape
    pen, inv = np.float32(penalty), np.float32(1.0 / penalty)
    for r in range(R):
        if active is not None and int(active[r]) == 0:
            continue
        h = [int(hist[r, i]) for i in range(t)]
        if float(pen) != 1.0:
            done = set()
            for w in h:
                if w in done or not (0 <= w < V):
                    continue
                done.add(w)
                z = np.float32(out[r, w].item())
                with np.errstate(all="ignore"):
                    out[r, w] = float(z * inv if z > 0 else z * pen)
        banned = []
        if n >= 1 and t >= n - 1:
            last = tuple(h[t - n + 1:t])
            for i in range(0, t - n + 1):
                if tuple(h[i:i + n - 1]) == last:
                    banned.append(h[i + n - 1])
        if t < min_len:
            banned.append(eos)
        banned += list(suppress)
        for w in banned:
            if 0 <= w < V:
                out[r, w] = -INF
    return out


def special_logits(R, V, g):
    """random rows with the SPECIAL values on the low columns (where the histories' tokens live), shifted per row"""
    z = torch.randn((R, V), generator=g) * 3
    for r in range(R):
        for j, v in enumerate(SPECIAL):
            c = (j + r) % max(len(SPECIAL), 1)
            if c < V:
                z[r, c] = v
    return z


def hand_histories(V, t):
    """histories of length t built to break things (token ids a, b, c, d are small columns, so they hit the SPECIAL values)"""
    a, b, c, d = 1 % V, 2 % V, 3 % V, 4 % V
    base = {
        "one_token": [a],
        "period2": [a, b],
        "period3": [a, b, c],
        "overlap": [a, a, a, b, a, a, a, c, a, a, a, d],          # the suffix (a, a) matches at overlapping positions, three followers
        "outside": [-1, c, V, d, -1, a, V, b],                    # ids outside [0, V) match in the comparison and touch no column
        "outside_only": [-1, V],
        "eos_inside": [b, V - 1, b],
    }
    return {k: (v * (t // len(v) + 1))[:t] for k, v in base.items()}


def history_rows(R, V, t, g, width=None):
    """int64 [R, width]: the hand-made histories first, then random ones over a four-token alphabet (many repeats); the columns
    behind t hold a token that would change the answer if the kernel read it"""
    width = max(t, 1) + 2 if width is None else width
    hist = torch.full((R, width), 5 % V, dtype=torch.int64)
    hands = list(hand_histories(V, t).values())
    for r in range(R):
        if r < len(hands):
            row = hands[r]
        else:
            row = torch.randint(0, min(V, 4), (t,), generator=g).tolist()
        if t:
            hist[r, :t] = torch.tensor(row, dtype=torch.int64)
    return hist


def settings(V, t, R):
    """(penalty, n, min_len, suppress, active) for every n in 0..4 x penalty in 0.5 / 1.0 / 1.3; the other controls rotate:
    min_len 0, t (t == m: off) and t + 1 (t == m - 1: on); the list off, with duplicates + ids outside [0, V), and with eos; the
    active mask off and with some rows off"""
    eos = V - 1
    lists = [(), (2 % V, 2 % V, -1, V, V + 7, 0), (eos, 3 % V, eos)]
    out = []
    i = 0
    for n in (0, 1, 2, 3, 4):
        for pen in (0.5, 1.0, 1.3):
            act = None
            if i % 2 == 1:
                act = torch.ones(R, dtype=torch.bool)
                act[::3] = False
            out.append((pen, n, (0, t, t + 1)[i % 3], lists[(i // 3 + i) % 3], act))
            i += 1
    return out


def host_law(logits, hist, t, pen, n, min_len, sup, eos, act):
    c = decode.Constraints(repetition_penalty=pen, no_repeat_ngram_size=n, min_length=min_len, suppress_tokens=sup)
    return decode.constrain_rows_host(logits, hist, t, c, eos, act)


@pytest.mark.parametrize("V", [5, 37, 1001])
def test_host_law_equals_the_naive_restatement(V):
    g = torch.Generator().manual_seed(V)
    seen_ban = seen_pen = 0
    for R in (1, 3, 12):
        logits = special_logits(R, V, g)
        for t in (0, 1, 2, 3, 17, 63):
            hist = history_rows(R, V, t, g)
            for pen, n, min_len, sup, act in settings(V, t, R):
                keep = logits.clone()
                got = host_law(logits, hist, t, pen, n, min_len, sup, V - 1, act)
                want = naive_rows(logits, hist, t, pen, n, min_len, sup, V - 1, act)
                assert same_bits(got, want), (V, R, t, pen, n, min_len, sup)
                assert same_bits(logits, keep)                                    # the input is not modified
                if act is not None:
                    assert same_bits(got[~act], logits[~act])
                seen_ban += int(((got == -INF) & (logits != -INF)).sum())
                seen_pen += int(((got != logits) & (got != -INF)).sum())
    assert seen_ban > 0 and seen_pen > 0


def test_host_law_hand_cases():
    V, eos = 10, 9
    z = torch.tensor([[1.0, 2.0, -2.0, 0.0, -0.0, -INF, 4.0, 8.0, 3.0, 5.0]])
    law = lambda h, **kw: decode.constrain_rows_host(z, torch.tensor([h], dtype=torch.int64) if h else None, len(h),
                                                     decode.Constraints(**kw), eos)[0]
    # the penalty once per distinct token; positive divided, negative multiplied, zeros keep their sign, -inf stays
    out = law([1, 1, 1, 2, 3, 4, 5, 2], repetition_penalty=2.0)
    assert out.tolist()[:3] == [1.0, 1.0, -4.0] and out[5] == -INF
    assert same_bits(out[3:5], z[0, 3:5] * 2)
    assert torch.equal(out[6:], z[0, 6:])
    # period 2 with bigrams: after ... 7 8 7 the continuation 8 is banned (and only it)
    out = law([7, 8, 7], no_repeat_ngram_size=2)
    assert (out == -INF).nonzero().flatten().tolist() == [5, 8]
    # overlapping matches of the suffix (6, 6): followers 6 and 7
    out = law([6, 6, 6, 7, 6, 6], no_repeat_ngram_size=3)
    assert (out == -INF).nonzero().flatten().tolist() == [5, 6, 7]
    # n - 1 > t: nothing; n - 1 == t: nothing (no earlier n-gram); n == 1: the whole history
    assert torch.equal(law([1], no_repeat_ngram_size=3), z[0]) and torch.equal(law([1, 2], no_repeat_ngram_size=3), z[0])
    assert (law([1, 2, 1], no_repeat_ngram_size=1) == -INF).nonzero().flatten().tolist() == [1, 2, 5]
    # ids outside [0, V) match in the comparison and touch nothing
    out = law([-1, 6, -1, 7, -1], no_repeat_ngram_size=2, repetition_penalty=2.0)
    assert (out == -INF).nonzero().flatten().tolist() == [5, 6, 7]
    out = law([6, 10, 6], no_repeat_ngram_size=2, repetition_penalty=2.0)
    assert (out == -INF).nonzero().flatten().tolist() == [5] and out[6] == 2.0
    # a banned token that is also penalised is -inf; min_length at t = m - 1 and t = m; the list
    assert law([7, 8, 7], no_repeat_ngram_size=2, repetition_penalty=1.3)[8] == -INF
    assert law([1, 2], min_length=3)[eos] == -INF and law([1, 2, 3], min_length=3)[eos] == 5.0
    out = law([], suppress_tokens=(0, 0, 12, -4, eos))
    assert (out == -INF).nonzero().flatten().tolist() == [0, 5, 9]


def test_constraints_validates_its_fields():
    c = decode.Constraints()
    assert c.off and c.logits_off and c.inv_penalty == 1.0 and c.penalty == 1.0
    assert (c.repetition_penalty, c.no_repeat_ngram_size, c.min_length, c.suppress_tokens, c.length_penalty) == (1.0, 0, 0, (), 0.0)
    c = decode.Constraints(repetition_penalty=1.3, no_repeat_ngram_size=3, min_length=5, suppress_tokens=[100, 103, 100], length_penalty=0.7)
    assert not c.off and c.suppress_tokens == (100, 103, 100)
    assert c.inv_penalty == f32(1 / 1.3) and c.penalty == f32(1.3)
    for kw in ({"repetition_penalty": 1.2}, {"no_repeat_ngram_size": 1}, {"min_length": 1}, {"suppress_tokens": (0,)}):
        assert not decode.Constraints(**kw).off and not decode.Constraints(**kw).logits_off
    lp = decode.Constraints(length_penalty=1.0)
    assert not lp.off and lp.logits_off                            # length_penalty alone: no launch, only the final pick
    assert decode.Constraints(suppress_tokens=None).off and decode.Constraints(suppress_tokens=torch.tensor([4, 5])).suppress_tokens == (4, 5)
    for p in (0.0, -1.0, INF, float("nan"), 1e-60, 1e60):
        with pytest.raises(ValueError, match="repetition_penalty"):
            decode.Constraints(repetition_penalty=p)
    for n in (-1, 2.5):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            decode.Constraints(no_repeat_ngram_size=n)
    for n in (-1, 0.5):
        with pytest.raises(ValueError, match="min_length"):
            decode.Constraints(min_length=n)
    for s in ((1.5,), (2 ** 31,)):
        with pytest.raises(ValueError, match="suppress_tokens"):
            decode.Constraints(suppress_tokens=s)
    for a in (INF, -INF, float("nan")):
        with pytest.raises(ValueError, match="length_penalty"):
            decode.Constraints(length_penalty=a)


def test_library_exports_the_symbol_and_the_binding_knows_it():
    from valor_amd import kernels as K, lib
    so = lib.load()
    assert hasattr(so, "valor_logits_constrain") and len(lib.SIGNATURES["valor_logits_constrain"]) == 18
    assert callable(K.logits_constrain)
    if not torch.cuda.is_available():
        with pytest.raises(lib.ValorHipError):                     # no CPU fallback
            K.logits_constrain(torch.zeros(2, 8), None, 0, 3)


def test_logits_constrain_validates_arguments_without_gpu():
    from valor_amd import lib
    so = lib.load()
    f = (ctypes.c_float * 64)()
    i64 = (ctypes.c_int64 * 64)()
    i32 = (ctypes.c_int32 * 4)()
    u8 = (ctypes.c_uint8 * 4)()

    def call(R=4, V=16, ld=16, t=3, eos=3, pen=1.3, n=2, min_len=0, logits=f, hist=i64, ss=8, sk=0, b=4, sup=i32, ns=4, act=u8):
        return so.valor_logits_constrain(None, logits, ld, R, V, hist, ss, sk, b, t, eos, pen, 1.0 / pen if pen else 0.0, n, min_len, sup,
                                         ns, act)
    assert call(R=0) == 0 and call(R=0, logits=None, hist=None) == 0             # no rows: no-op, nothing is launched
    assert call(logits=None) == -1 and call(hist=None) == -1
    assert call(R=-1) == -1 and call(V=0) == -1 and call(ld=15) == -1 and call(t=-1) == -1 and call(t=513) == -1
    assert call(n=-1) == -1 and call(min_len=-1) == -1
    assert call(eos=16) == -1 and call(eos=-1) == -1
    for bad in (0.0, -1.0, INF, float("nan")):
        assert call(pen=bad) == -1, bad
    assert call(ns=-1) == -1 and call(sup=None) == -1
    assert call(b=0) == -1 and call(ss=-1) == -1 and call(sk=-8) == -1


def test_generate_argument_errors_and_signatures():
    import inspect
    m = VALOR(None, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu")
    qa = lambda **kw: decode.generate_qa(m, {}, ["tv"], torch.zeros((1, 4), dtype=torch.long), **kw)
    cap = lambda **kw: decode.generate_cap(m, {}, ["tv"], **kw)
    for gen in (cap, qa):
        with pytest.raises(ValueError, match="repetition_penalty"):
            gen(repetition_penalty=0)
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            gen(no_repeat_ngram_size=-2)
        with pytest.raises(ValueError, match="min_length"):
            gen(mode="sample", min_length=-1)
        with pytest.raises(ValueError, match="length_penalty"):
            gen(length_penalty=INF)
    with pytest.raises(ValueError, match="mode"):
        qa(mode="beam")
    with pytest.raises(ValueError, match="mode='sample'"):
        qa(top_k=3)
    with pytest.raises(ValueError, match="top_p"):
        qa(mode="sample", top_p=0.0)
    bad = VALOR({"generation_no_repeat_ngram_size": -1}, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):           # the model's options go through the same validation
        decode.generate_cap(bad, {}, ["tv"])
    names = ("repetition_penalty", "no_repeat_ngram_size", "min_length", "suppress_tokens", "length_penalty")
    for fn in (decode.generate_cap, decode.generate_qa):
        p = inspect.signature(fn).parameters
        assert all(p[k].default is None for k in names)
    for fn in (decode.decode_greedy, decode.decode_beam, decode.decode_sample, decode._decode_groups):
        assert inspect.signature(fn).parameters["constraints"].default is None
