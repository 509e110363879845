"""Fixture of the device caption reward (tests/golden/scst_reward.pt) from the UNMODIFIED reference: its scorer.cider.Cider and
scorer.bleu.Bleu are imported and called on a seeded corpus (as tests/test_scst_cpu.py does); nothing of their text is copied. Only data
is stored, as numbers and tensors (pack / load below): the corpus (about 60 clips with 1-20 references of 3-15 token ids), the clips the document frequency is counted over (a
subset: n-grams of the other clips have no df entry), an [R, L] id matrix whose rows cover the six hypothesis kinds below -- each
followed by its eos and then by tokens that WOULD score if they were counted --, the rows' clip ids, and the reference's per-row CIDEr-D
and BLEU-4 (fp64).

    python tools/make_reward_goldens.py            # needs the reference tree (oracle/ref_harness.py); writes tests/golden/

The six kinds (tests/test_scst_cpu._hyps): empty; longer than every reference; n-grams with no df entry; repeated n-grams; a reference
itself; a prefix of a reference plus noise. The helpers below are what tests/test_reward_*.py import: fixture and tests use one
definition of the corpus and of the padded matrix."""
import os
import sys
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scst_reward.pt")
EOS = 102
CASE = dict(seed=0, clips=60, df_clips=45, rows=240, vocab=40)


def corpus(seed=0, clips=60, vocab=40):
    """{clip id: 1-20 references of 3-15 token ids in [1000, 1000 + vocab)}"""
    rng = np.random.default_rng(seed)
    return {f"clip{c}": [rng.integers(1000, 1000 + vocab, size=int(rng.integers(3, 16))).tolist() for _ in range(int(rng.integers(1, 21)))]
            for c in range(clips)}


def hyps_six_kinds(refs, ids, seed=1, vocab=40):
    """one hypothesis per id, kind = row % 6 (see the module docstring)"""
    rng = np.random.default_rng(seed)
    out = []
    for i, cid in enumerate(ids):
        kind = i % 6
        if kind == 0:
            h = []
        elif kind == 1:
            h = rng.integers(1000, 1000 + vocab, size=max(len(r) for r in refs[cid]) + 5).tolist()
        elif kind == 2:
            h = rng.integers(5000, 5010, size=int(rng.integers(1, 12))).tolist()
        elif kind == 3:
            w = int(rng.integers(1000, 1000 + vocab))
            h = [w, w + 1] * int(rng.integers(2, 6))
        elif kind == 4:
            h = list(refs[cid][0])
        else:
            r = list(refs[cid][int(rng.integers(len(refs[cid])))])
            h = r[:int(rng.integers(1, len(r) + 1))] + rng.integers(1000, 1000 + vocab, size=int(rng.integers(0, 5))).tolist()
        out.append(h)
    return out


def pad_rows(hyps, L, eos=EOS, seed=3, vocab=40):
    """int64 [R, L]: every hypothesis, its eos, then tokens of the corpus' vocabulary (they would score if they were counted)"""
    rng = np.random.default_rng(seed)
    m = rng.integers(1000, 1000 + vocab, size=(len(hyps), L))
    for r, h in enumerate(hyps):
        assert len(h) <= L
        m[r, :len(h)] = h
        if len(h) < L:
            m[r, len(h)] = eos
    return m.astype(np.int64)


def make_case(seed, clips, df_clips, rows, vocab):
    refs = corpus(seed, clips, vocab)
    df_ids = list(refs)[:df_clips]
    rng = np.random.default_rng(seed + 2)
    ids = [list(refs)[int(rng.integers(len(refs)))] for _ in range(rows)]
    hyps = hyps_six_kinds(refs, ids, seed + 1, vocab)
    return refs, df_ids, ids, hyps, pad_rows(hyps, max(len(h) for h in hyps) + 3, seed=seed + 3, vocab=vocab)


def generate():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    from scorer.bleu import Bleu
    from scorer.cider import Cider
    sys.path.insert(0, ROOT)
    from valor_amd import scst
    refs, df_ids, ids, hyps, seq = make_case(**CASE)
    assert scst.hypotheses(seq, EOS) == hyps                                   # the matrix says what the lists say
    df, ref_len = scst.document_frequency(refs, df_ids)                        # the rule of precompute_df_reflen_for_cider (tests/test_scst_cpu.py)
    gts = [refs[i] for i in ids]
    _, cider = Cider(document_frequency=defaultdict(int, df), ref_len=ref_len).compute_score(gts, hyps)
    _, bleu = Bleu().compute_score(gts, hyps)
    return dict(case=CASE, eos=EOS, refs=refs, df_ids=df_ids, ids=ids, seq=torch.from_numpy(seq),
                cider=torch.tensor(np.asarray(cider, dtype=np.float64)), bleu4=torch.tensor(np.asarray(bleu[-1], dtype=np.float64)))


def pack(fix):
    """the fixture as numbers and tensors only (torch.load(weights_only=True) reads it): the references as a CSR of int16 tokens (clip c =
    references clip_ptr[c] .. clip_ptr[c + 1], reference q = tokens ref_ptr[q] .. ref_ptr[q + 1]; clip c is called 'clip<c>'), the df clips
    as their count (the first ones), the rows' clips as numbers, the id matrix as int16"""
    names = list(fix["refs"])
    assert names == [f"clip{c}" for c in range(len(names))] and fix["df_ids"] == names[:len(fix["df_ids"])]
    flat = [r for n in names for r in fix["refs"][n]]
    assert 0 <= min(min(r) for r in flat) and max(max(r) for r in flat) < 2 ** 15 and 0 <= int(fix["seq"].min()) and int(fix["seq"].max()) < 2 ** 15
    return dict(case=dict(fix["case"]), eos=int(fix["eos"]), df_clips=len(fix["df_ids"]),
                clip_ptr=torch.tensor(np.cumsum([0] + [len(fix["refs"][n]) for n in names]), dtype=torch.int32),
                ref_ptr=torch.tensor(np.cumsum([0] + [len(r) for r in flat]), dtype=torch.int32),
                ref_tokens=torch.tensor([t for r in flat for t in r], dtype=torch.int16),
                ids=torch.tensor([names.index(i) for i in fix["ids"]], dtype=torch.int32), seq=fix["seq"].to(torch.int16),
                cider=fix["cider"], bleu4=fix["bleu4"])


def load(path=GOLDEN):
    """the fixture file -> what generate() returns: refs {clip id: token-id lists}, df_ids, ids (one clip id per row), seq int64 [R, L],
    eos, cider / bleu4 fp64 [R]"""
    p = torch.load(path, weights_only=True)
    clip_ptr, ref_ptr, tok = p["clip_ptr"].tolist(), p["ref_ptr"].tolist(), p["ref_tokens"].tolist()
    names = [f"clip{c}" for c in range(len(clip_ptr) - 1)]
    refs = {n: [tok[ref_ptr[q]:ref_ptr[q + 1]] for q in range(clip_ptr[c], clip_ptr[c + 1])] for c, n in enumerate(names)}
    return dict(case=p["case"], eos=p["eos"], refs=refs, df_ids=names[:p["df_clips"]], ids=[names[c] for c in p["ids"].tolist()],
                seq=p["seq"].to(torch.int64), cider=p["cider"], bleu4=p["bleu4"])


def main():
    fix = generate()
    torch.save(pack(fix), GOLDEN)
    back = load()
    assert all(back[k] == fix[k] for k in ("case", "eos", "refs", "df_ids", "ids")) and all(torch.equal(back[k], fix[k]) for k in ("seq", "cider", "bleu4"))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes;", len(fix["ids"]), "rows x", fix["seq"].shape[1], "; CIDEr-D", float(fix["cider"].min()), "..",
          float(fix["cider"].max()), "BLEU-4", float(fix["bleu4"].min()), "..", float(fix["bleu4"].max()))


if __name__ == "__main__":
    main()
