"""Fixture of the caption evaluation metrics (tests/golden/cap_metrics.pt) from the UNMODIFIED reference: its Bleu(4), Rouge() and Cider()
(cococaption/pycocoevalcap/{bleu,rouge,cider}; the submodules are imported, eval.py itself pulls in the Java wrappers) are called on a
seeded corpus whose "words" are decimal integers joined by single spaces; nothing of their text is copied. Only data is stored, as
numbers and tensors (pack / load below): the corpus as an int16 CSR, the id matrix, the rows' clips, the reference's per-clip Bleu_1..4,
ROUGE-L and CIDEr (fp64) and the six corpus values.

    python tools/make_capeval_goldens.py            # needs the reference tree (oracle/ref_harness.py); writes tests/golden/

The corpus: the 60 clips of tools/make_reward_goldens.py (1-20 references of 3-15 symbols), one clip with 70 references (more than a
wave has lanes, and more n-gram entries than the kernel stages in LDS), one clip with a reference of 200 symbols, and six clips with
long references for the hypotheses of exactly 1, 63, 64, 65, 127 and 128 symbols. EVERY CLIP IS EVALUATED EXACTLY ONCE (the CIDEr document
frequency is counted over the evaluated clips). The first 60 hypotheses are the six kinds of make_reward_goldens.hyps_six_kinds (one of
them empty: the reference's scorers accept it); every hypothesis is followed by the end mark and then by symbols that WOULD score if
they were counted. The seed is chosen so that no corpus value * 100 lies within 1e-6 of a rounding boundary at two decimals (asserted
on the reference's numbers alone): the rounded dict can then be compared for equality.
The helpers below are what tests/test_capeval_*.py import: fixture and tests use one definition of the corpus."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_reward_goldens import EOS, corpus as reward_corpus, hyps_six_kinds, pad_rows  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "cap_metrics.pt")
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
EDGE_LENGTHS = (1, 63, 64, 65, 127, 128)
CASE = dict(seed=0, clips=60, vocab=40)
L = 128


def corpus(seed=0, clips=60, vocab=40):
    """{clip id: references}: `clips` clips of the reward corpus, 'many' (70 references), 'long' (a reference of 200 symbols among
    three), and 'edge<n>' for n in EDGE_LENGTHS (four references of 40-140 symbols)"""
    refs = reward_corpus(seed, clips, vocab)
    rng = np.random.default_rng(seed + 10)
    word = lambda n: rng.integers(1000, 1000 + vocab, size=int(n)).tolist()
    refs["many"] = [word(rng.integers(3, 16)) for _ in range(70)]
    refs["long"] = [word(200), word(9), word(130)]
    for n in EDGE_LENGTHS:
        refs[f"edge{n}"] = [word(rng.integers(40, 141)) for _ in range(4)]
    return refs


def hypotheses(refs, seed=0, vocab=40):
    """one hypothesis per clip, in the order of `refs`"""
    ids = list(refs)
    base = [i for i in ids if i.startswith("clip")]
    hyps = hyps_six_kinds(refs, base, seed + 1, vocab)
    rng = np.random.default_rng(seed + 11)
    word = lambda n: rng.integers(1000, 1000 + vocab, size=int(n)).tolist()
    r = refs["many"][69]
    hyps.append(r[:4] + word(3) + r[4:])                                       # 'many': its last reference with noise in the middle
    hyps.append(refs["long"][0][40:140] + word(20))                            # 'long': 100 symbols of the long reference, then noise
    for n in EDGE_LENGTHS:
        r = refs[f"edge{n}"][1]
        h = [w if rng.random() < 0.6 else int(rng.integers(1000, 1000 + vocab)) for w in (r * 4)[:n]]
        hyps.append(h)
    assert len(hyps) == len(ids) and [len(h) for h in hyps[-len(EDGE_LENGTHS):]] == list(EDGE_LENGTHS)
    return ids, hyps


def make_case(seed, clips, vocab):
    refs = corpus(seed, clips, vocab)
    ids, hyps = hypotheses(refs, seed, vocab)
    return refs, ids, hyps, pad_rows(hyps, L, seed=seed + 3, vocab=vocab)


def boundary_margin(values):
    """the smallest distance of a value * 100 from a rounding boundary at two decimals (k + 0.5) / 100"""
    return min(abs((v * 1e4) % 1.0 - 0.5) / 100 for v in values)


def generate():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    from cococaption.pycocoevalcap.bleu.bleu import Bleu
    from cococaption.pycocoevalcap.cider.cider import Cider
    from cococaption.pycocoevalcap.rouge.rouge import Rouge
    sys.path.insert(0, ROOT)
    from valor_amd import scst
    refs, ids, hyps, seq = make_case(**CASE)
    assert scst.hypotheses(seq, EOS) == hyps                                   # the matrix says what the lists say
    text = lambda words: " ".join(str(w) for w in words)
    gts = {i: [text(r) for r in refs[i]] for i in ids}
    res = {i: [text(h)] for i, h in zip(ids, hyps)}
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")                     # the reference's Bleu prints every clip's integers
    try:
        bleu, bleus = Bleu(4).compute_score(gts, res)
    finally:
        sys.stdout.close()
        sys.stdout = stdout
    rouge, rouges = Rouge().compute_score(gts, res)
    cider, ciders = Cider().compute_score(gts, res)
    corpus_values = [float(b) for b in bleu] + [float(rouge), float(cider)]
    assert boundary_margin(corpus_values) > 1e-6, (corpus_values, "choose another seed")
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return dict(case=CASE, eos=EOS, refs=refs, ids=ids, seq=torch.from_numpy(seq), bleu=f64(bleus).t().contiguous(), rouge=f64(rouges),
                cider=f64(ciders), corpus=f64(corpus_values))


def pack(fix):
    """the fixture as numbers and tensors only (torch.load(weights_only=True) reads it): the references as a CSR of int16 symbols in the
    order of corpus() (the clip names follow from the case), the rows' clips as numbers, the id matrix as int16"""
    names = list(fix["refs"])
    flat = [r for n in names for r in fix["refs"][n]]
    assert 0 <= min(min(r) for r in flat) and max(max(r) for r in flat) < 2 ** 15 and 0 <= int(fix["seq"].min()) and int(fix["seq"].max()) < 2 ** 15
    return dict(case=dict(fix["case"]), eos=int(fix["eos"]),
                clip_ptr=torch.tensor(np.cumsum([0] + [len(fix["refs"][n]) for n in names]), dtype=torch.int32),
                ref_ptr=torch.tensor(np.cumsum([0] + [len(r) for r in flat]), dtype=torch.int32),
                ref_tokens=torch.tensor([t for r in flat for t in r], dtype=torch.int16),
                ids=torch.tensor([names.index(i) for i in fix["ids"]], dtype=torch.int32), seq=fix["seq"].to(torch.int16),
                bleu=fix["bleu"], rouge=fix["rouge"], cider=fix["cider"], corpus=fix["corpus"])


def load(path=GOLDEN):
    """the fixture file -> what generate() returns: refs {clip id: symbol lists}, ids (one clip id per row), seq int64 [R, L], eos,
    bleu fp64 [R, 4], rouge / cider fp64 [R], corpus fp64 [6] in the order of KEYS"""
    p = torch.load(path, weights_only=True)
    clip_ptr, ref_ptr, tok = p["clip_ptr"].tolist(), p["ref_ptr"].tolist(), p["ref_tokens"].tolist()
    names = list(corpus(**p["case"]))
    assert len(names) == len(clip_ptr) - 1
    refs = {n: [tok[ref_ptr[q]:ref_ptr[q + 1]] for q in range(clip_ptr[c], clip_ptr[c + 1])] for c, n in enumerate(names)}
    return dict(case=p["case"], eos=p["eos"], refs=refs, ids=[names[c] for c in p["ids"].tolist()], seq=p["seq"].to(torch.int64),
                bleu=p["bleu"], rouge=p["rouge"], cider=p["cider"], corpus=p["corpus"])


def main():
    fix = generate()
    torch.save(pack(fix), GOLDEN)
    back = load()
    assert all(back[k] == fix[k] for k in ("case", "eos", "refs", "ids")) and all(torch.equal(back[k], fix[k]) for k in ("seq", "bleu", "rouge", "cider", "corpus"))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes;", len(fix["ids"]), "rows x", fix["seq"].shape[1], ";",
          dict(zip(KEYS, [round(v * 100, 2) for v in fix["corpus"].tolist()])), "margin", boundary_margin(fix["corpus"].tolist()))


if __name__ == "__main__":
    main()
