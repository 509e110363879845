"""CPU: the flat tables of the device caption scorer (valor_amd.scst.reward_tables / DeviceCaptionScorer) -- key packing, sorted unique
lists, idf bits --, the numpy walker of those tables (scst.reward_from_tables) against the host CaptionScorer, the constructor's errors,
and the argument checks of valor_caption_reward without a GPU.

Tolerance of every fp64 comparison against the host scorer: rtol 1e-9, atol 1e-12. Every summed term is non-negative and a sum has fewer
than ~1e3 terms, so a reordered fp64 sum moves by ~1e-13 relative; exp / sqrt / pow differ between implementations by a few ulp; 1e-9
leaves four orders of margin and is six orders tighter than the fp32 rounding the only consumer applies. atol covers the rows whose
exact score is 0 or ~1e-4 (BLEU with no match). No row is excluded."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_reward_goldens import EOS, corpus, hyps_six_kinds, load, pad_rows  # noqa: E402  (one definition for fixture and tests)
from valor_amd import scst  # noqa: E402

RTOL, ATOL = 1e-9, 1e-12


def test_key_packing_round_trips():
    rng = np.random.default_rng(0)
    seen = {}
    for _ in range(2000):
        g = tuple(int(x) for x in rng.integers(0, scst.MAX_TOKEN + 1, size=int(rng.integers(1, 5))))
        k = scst.pack_key(g)
        assert 0 < k < 2 ** 64 and scst.unpack_key(k) == g
        assert seen.setdefault(k, g) == g                                      # collision-free
    assert scst.unpack_key(scst.pack_key((0,))) == (0,) and scst.unpack_key(scst.pack_key((0, 0, 0, 0))) == (0, 0, 0, 0)
    assert scst.pack_key((scst.MAX_TOKEN,) * 4) < 0xFFFF_FFFF_FFFF_FFFF        # the unknown code is in no valid key
    for bad in ((), (1, 2, 3, 4, 5), (scst.MAX_TOKEN + 1,), (-1,), (65535,)):
        with pytest.raises(ValueError):
            scst.pack_key(bad)


def test_tables_are_sorted_unique_and_hold_the_scorers_numbers():
    refs = corpus()
    sc = scst.CaptionScorer(refs, df_ids=list(refs)[:45])
    T = scst.reward_tables(sc)
    strictly = lambda a: bool((a[1:] > a[:-1]).all())
    assert T["g_keys"].dtype == np.uint64 and strictly(T["g_keys"]) and len(T["g_keys"]) == len(sc.df)
    for k, idf in zip(T["g_keys"], T["g_idf"]):
        want = sc.ref_len - np.log(max(1.0, sc.df[scst.unpack_key(k)]))
        assert idf == want                                                     # bit for bit
    assert T["clips"] == list(refs) and T["ref_len"] == sc.ref_len
    q = 0
    for c, cid in enumerate(T["clips"]):
        assert T["clip_ref_ptr"][c + 1] - T["clip_ref_ptr"][c] == len(refs[cid])
        for (vec, norm, length), r in zip(sc._cider_refs[cid], refs[cid]):
            lo, hi = T["ref_key_ptr"][q], T["ref_key_ptr"][q + 1]
            keys = T["ref_keys"][lo:hi]
            assert strictly(keys) and hi - lo == sum(len(d) for d in vec)
            for k, v in zip(keys, T["ref_vals"][lo:hi]):
                g = scst.unpack_key(k)
                assert vec[len(g) - 1][g] == v
            assert list(T["ref_norm"][q]) == [float(x) for x in norm]
            assert T["ref_bigrams"][q] == length == max(len(r) - 1, 0) and T["ref_tokens"][q] == len(r)
            q += 1
        b0, b1 = T["clip_bleu_ptr"][c], T["clip_bleu_ptr"][c + 1]
        assert strictly(T["bleu_keys"][b0:b1])
        assert {scst.unpack_key(k): int(n) for k, n in zip(T["bleu_keys"][b0:b1], T["bleu_cnt"][b0:b1])} == sc._bleu_refs[cid][1]
    assert q == len(T["ref_tokens"]) == T["clip_ref_ptr"][-1]


def test_table_walker_equals_the_host_scorer():
    refs = corpus()
    sc = scst.CaptionScorer(refs, df_ids=list(refs)[:45])
    dsc = scst.DeviceCaptionScorer(sc)
    assert isinstance(sc.to_device(), scst.DeviceCaptionScorer)
    rng = np.random.default_rng(2)
    ids = [list(refs)[int(rng.integers(len(refs)))] for _ in range(240)]
    hyps = hyps_six_kinds(refs, ids)
    seq = pad_rows(hyps, max(len(h) for h in hyps) + 2)
    idx = dsc.clip_index(ids)
    assert idx.dtype == np.int32 and [dsc.tables["clips"][i] for i in idx] == ids
    got, c, b = scst.reward_from_tables(dsc.tables, idx, seq, EOS, parts=True)
    want_c = np.array([sc.cider(i, h) for i, h in zip(ids, hyps)])
    want_b = np.array([sc.bleu4(i, h) for i, h in zip(ids, hyps)])
    np.testing.assert_allclose(c, want_c, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(b, want_b, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got, sc(ids, hyps), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(scst.reward_from_tables(dsc.tables, idx, seq, EOS), sc(ids, scst.hypotheses(seq, EOS)), rtol=RTOL, atol=ATOL)
    assert (c[::6] == 0).all() and np.ptp(c) > 1.0 and (c[4::6] > 0).all()
    # tokens outside the vocabulary match nothing, and two different ones stay two n-grams (the norms see the difference)
    odd = np.array([[1000, 70000, 80000, 1001, EOS, 1002], [1000, 70000, 70000, 1001, -5, 1002]], dtype=np.int64)
    np.testing.assert_allclose(scst.reward_from_tables(dsc.tables, idx[:2], odd, EOS), sc(ids[:2], scst.hypotheses(odd, EOS)), rtol=RTOL, atol=ATOL)


def test_constructor_and_lookup_errors():
    refs = corpus(clips=5)
    for bad in (scst.MAX_TOKEN + 1, 65535, 70000, -1):
        broken = dict(refs, extra=[[1000, bad, 1001]])
        with pytest.raises(ValueError):
            scst.DeviceCaptionScorer(broken)
    ok = scst.DeviceCaptionScorer(dict(refs, edge=[[0, scst.MAX_TOKEN, 7]]), df_ids=list(refs)[:3])
    assert ok.host.ref_len == np.log(3.0)
    with pytest.raises(KeyError):
        ok.clip_index(["clip0", "nowhere"])
    with pytest.raises(ValueError):
        scst.DeviceCaptionScorer(ok.host, df_ids=["clip0"])
    with pytest.raises(ValueError):
        scst.DeviceCaptionScorer(dict(refs, bare=[])).clip_index(["bare"])


def test_caption_reward_validates_arguments_without_gpu():
    from valor_amd import lib
    so = lib.load()
    assert "valor_caption_reward" in lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "valor_hip.h")).read()
    assert "int valor_caption_reward(" in hdr and "valor_reward_tables" in hdr and "max_generation_len" in hdr
    i64 = (ctypes.c_int64 * 1024)()
    i32 = (ctypes.c_int32 * 64)()
    f64 = (ctypes.c_double * 64)()
    buf = ctypes.addressof(i64)
    tab = lib.RewardTables()
    for k in lib.RewardTables.POINTERS:
        setattr(tab, k, buf)
    tab.ref_len, tab.n_global, tab.n_clips = 1.0, 4, 2
    assert ctypes.sizeof(tab) == 12 * 8 + 8 + 2 * 4

    def call(R=4, L=30, ld=30, eos=102, vocab=30522, seq=i64, clip=i32, tables=tab, reward=f64):
        t = None if tables is None else ctypes.addressof(tables)
        return so.valor_caption_reward(None, seq, ld, R, L, eos, vocab, clip, t, reward, None, None)
    assert call(R=-1) == -1 and call(L=0) == -1 and call(L=129, ld=129) == -1 and call(ld=29) == -1
    assert call(vocab=65535) == -1 and call(vocab=0) == -1 and call(eos=30522) == -1 and call(eos=-1) == -1
    assert call(seq=None) == -1 and call(clip=None) == -1 and call(tables=None) == -1 and call(reward=None) == -1
    for k in lib.RewardTables.POINTERS:
        broken = lib.RewardTables.from_buffer_copy(tab)
        setattr(broken, k, None)
        assert call(tables=broken) == -1, k
    assert call(R=0) == 0 and call(R=0, seq=None, reward=None) == 0            # no rows: no-op
    assert call(R=0, L=128, ld=128, vocab=65534, eos=65533) == 0               # the largest geometry is inside the domain


def test_table_walker_equals_the_reference_fixture():
    """tests/golden/scst_reward.pt (tools/make_reward_goldens.py): the unmodified reference's per-row CIDEr-D and BLEU-4"""
    fix = load()                                                               # numbers and tensors only: torch.load(weights_only=True)
    dsc = scst.DeviceCaptionScorer(fix["refs"], df_ids=fix["df_ids"])
    _, c, b = scst.reward_from_tables(dsc.tables, dsc.clip_index(fix["ids"]), fix["seq"].numpy(), fix["eos"], parts=True)
    np.testing.assert_allclose(c, fix["cider"].numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(b, fix["bleu4"].numpy(), rtol=RTOL, atol=ATOL)
    assert len(c) == 240 and (c[::6] == 0).all() and np.ptp(c) > 1.0


def test_reward_tables_struct_is_one_layout_in_header_binding_and_kernel():
    """valor_reward_tables: the ctypes binding lists the header's fields in the header's order with the header's types (so every offset
    agrees, not only the size), and the kernel has no definition of its own: it includes the header"""
    import re
    from valor_amd import lib
    hdr = open(os.path.join(ROOT, "include", "valor_hip.h")).read()
    body = re.search(r"typedef struct valor_reward_tables \{(.*?)\} valor_reward_tables;", hdr, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(const\s+\w+\s*\*|\w+)\s*(\w+(?:\s*,\s*\w+)*)", decl)
        assert m, decl
        ctype = "ptr" if "*" in m.group(1) else m.group(1)
        fields += [(n.strip(), ctype) for n in m.group(2).split(",")]
    ctypes_of = {"ptr": ctypes.c_void_p, "double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(n, ctypes_of[t]) for n, t in fields] == [(n, t) for n, t in lib.RewardTables._fields_]
    assert tuple(n for n, t in fields if t == "ptr") == lib.RewardTables.POINTERS
    off = 0
    for n, t in fields:                                                        # natural alignment, no padding: offsets are running sums
        assert getattr(lib.RewardTables, n).offset == off, n
        off += ctypes.sizeof(ctypes_of[t])
    assert off == ctypes.sizeof(lib.RewardTables)
    src = open(os.path.join(ROOT, "valor_amd", "csrc", "reward.hip")).read()
    assert '#include "../../include/valor_hip.h"' in src and not re.search(r"\bstruct\s+\w+\s*\{", src)
    # scst.reward_tables fills every pointer field by name
    T = scst.reward_tables(scst.CaptionScorer(corpus(clips=3)))
    assert set(lib.RewardTables.POINTERS) <= set(T) and {"ref_len", "clips"} <= set(T)


def test_device_scorer_names_the_geometry_it_does_not_take():
    """check(): a vocabulary above 65534 entries, an eos outside the vocabulary and rows wider than MAX_ROW_LEN raise ValueError before
    anything reaches the library (VALOR.forward_cap_scst calls it before decoding)"""
    dsc = scst.DeviceCaptionScorer(corpus(clips=3))
    assert dsc.check(EOS) == scst.MAX_VOCAB and dsc.check(EOS, 30522, 30) == 30522 and dsc.check(65533, 65534, scst.MAX_ROW_LEN) == 65534
    for eos, vocab, L in ((EOS, 65535, 30), (EOS, 0, 30), (30522, 30522, 30), (-1, 30522, 30), (65534, None, 30), (EOS, 30522, 129), (EOS, 30522, 0)):
        with pytest.raises(ValueError):
            dsc.check(eos, vocab, L)
