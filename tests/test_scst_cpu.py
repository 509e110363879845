"""CPU: the SCST reward (valor_amd.scst.CaptionScorer) against the reference's own CIDEr-D / BLEU scorers (imported from the reference
tree where it is present, skipped elsewhere), its df / ref_len rule and annotation loader, the scst_finetuning option plumbing, and the
argument checks of the new entry points (valor_sample_tokens, valor_xent_weighted_bwd, valor_weighted_mean_f32) without a GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_harness  # noqa: E402
from valor_amd import scst, synth  # noqa: E402
from valor_amd.model.valor import VALOR  # noqa: E402

needs_ref = pytest.mark.skipif(not ref_harness.available(), reason="the reference tree is not present")


def _ref_scorers():
    if ref_harness.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REF_ROOT)
    from scorer.bleu import Bleu
    from scorer.cider import Cider
    from scorer.cider_scorer import cook_refs
    return Cider, Bleu, cook_refs


def _corpus(seed=0, clips=60, vocab=40):
    rng = np.random.default_rng(seed)
    refs = {}
    for c in range(clips):
        refs[f"clip{c}"] = [rng.integers(1000, 1000 + vocab, size=int(rng.integers(3, 16))).tolist() for _ in range(int(rng.integers(1, 21)))]
    return refs


def _hyps(refs, ids, seed=1, vocab=40):
    rng = np.random.default_rng(seed)
    hyps = []
    for i, cid in enumerate(ids):
        kind = i % 6
        if kind == 0:
            h = []                                                            # empty hypothesis
        elif kind == 1:
            h = rng.integers(1000, 1000 + vocab, size=max(len(r) for r in refs[cid]) + 5).tolist()      # longer than every reference
        elif kind == 2:
            h = rng.integers(5000, 5010, size=int(rng.integers(1, 12))).tolist()                      # n-grams with no df entry
        elif kind == 3:
            w = int(rng.integers(1000, 1000 + vocab))
            h = [w, w + 1] * int(rng.integers(2, 6))                                                    # repeated n-grams
        elif kind == 4:
            h = list(refs[cid][0])                                                                      # a reference itself
        else:
            r = list(refs[cid][int(rng.integers(len(refs[cid])))])
            h = r[:int(rng.integers(1, len(r) + 1))] + rng.integers(1000, 1000 + vocab, size=int(rng.integers(0, 5))).tolist()
        hyps.append(h)
    return hyps


@needs_ref
def test_cider_bleu_match_the_reference_scorers():
    Cider, Bleu, _ = _ref_scorers()
    refs = _corpus()
    df_ids = list(refs)[:45]                                 # df from a subset: n-grams of the other clips have no df entry
    sc = scst.CaptionScorer(refs, df_ids=df_ids)
    rng = np.random.default_rng(2)
    ids = [list(refs)[int(rng.integers(len(refs)))] for _ in range(240)]
    hyps = _hyps(refs, ids)
    gts = [refs[i] for i in ids]
    from collections import defaultdict
    df = defaultdict(int, sc.df)
    _, c_ref = Cider(document_frequency=df, ref_len=sc.ref_len).compute_score(gts, hyps)
    _, b_ref = Bleu().compute_score(gts, hyps)
    c_ours = np.array([sc.cider(i, h) for i, h in zip(ids, hyps)])
    b_ours = np.array([sc.bleu4(i, h) for i, h in zip(ids, hyps)])
    np.testing.assert_allclose(c_ours, np.asarray(c_ref), rtol=1e-12, atol=0)
    np.testing.assert_allclose(b_ours, np.asarray(b_ref[-1]), rtol=1e-12, atol=0)
    # the Scorer's reward: CIDEr-D + BLEU-4, weights [1, 1] (scorer/scorer.py:65-75)
    np.testing.assert_allclose(sc(ids, hyps), np.asarray(c_ref) + np.asarray(b_ref[-1]), rtol=1e-12, atol=0)
    assert (c_ours[::6] == 0).all() and np.ptp(c_ours) > 1.0


@needs_ref
def test_df_and_ref_len_follow_precompute_df_reflen_for_cider():
    """scorer/scorer.py:117-147 (restated: the module imports ipdb and cococaption): df = per n-gram the number of the listed clips whose
    cooked references contain it (the reference's cook_refs), ref_len = log(#listed clips with annotations)"""
    _, _, cook_refs = _ref_scorers()
    refs = _corpus(seed=5, clips=12)
    ids = [f"clip{c}" for c in (0, 2, 3, 7, 11)] + ["missing"]
    df_ref = {}
    n_clips = 0
    for cid in ids:
        if cid not in refs:
            continue
        n_clips += 1
        for g in set(g for r in cook_refs(refs[cid]) for g in r):
            df_ref[g] = df_ref.get(g, 0) + 1
    df, ref_len = scst.document_frequency(refs, ids)
    assert dict(df) == df_ref and ref_len == np.log(float(n_clips))


def test_from_annotations_reads_the_reference_layout(tmp_path):
    anns = {"annotations": [{"video_id": "a", "caption": "a man runs"}, {"video_id": "a", "caption": "a man is running"},
                            {"video_id": "b", "caption": "a dog barks"}, {"video_id": "c", "caption": "the cat sleeps"}]}
    (tmp_path / "ann.json").write_text(json.dumps(anns))
    (tmp_path / "ids.json").write_text(json.dumps(["a", "b"]))
    vocab = {}
    encode = lambda s: [vocab.setdefault(w, 2000 + len(vocab)) for w in s.split()]
    sc = scst.CaptionScorer.from_annotations(str(tmp_path / "ann.json"), str(tmp_path / "ids.json"), encode)
    assert set(sc.refs) == {"a", "b", "c"} and len(sc.refs["a"]) == 2          # references from every annotation
    assert sc.ref_len == np.log(2.0)                                           # df over the listed ids only
    the = (vocab["the"],)
    assert sc.df.get(the, 0) == 0 and sc.df[(vocab["a"],)] == 2
    r = sc(["a", "c"], [encode("a man runs"), encode("a cat")])
    assert r.shape == (2,) and r[0] > r[1] > 0


def test_hypotheses_cut_at_the_first_sep():
    seq = torch.tensor([[5, 6, 102, 7, 102], [102, 102, 102, 102, 102], [1, 2, 3, 4, 0]])
    assert scst.hypotheses(seq, 102) == [[5, 6], [], [1, 2, 3, 4, 0]]


def test_scst_without_a_scorer_raises():
    m = VALOR({"scst_finetuning": True}, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu")
    assert m.scst_finetuning and m.scorer is None
    with pytest.raises(ValueError, match="scorer"):
        m({"ids": ["x"]}, task="cap%tva%tv", compute_loss=True)
    assert not VALOR(None, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu").scst_finetuning


def test_scst_inputs_layout():
    """the loss pass's teacher-forced rows: [MASK] j at index L + 1 + j predicts w_j; labels up to and including the first [SEP]"""
    m = VALOR({"scst_finetuning": True}, spec=synth.tiny_spec(), dtype=torch.float32, device="cpu")
    seq = torch.tensor([[7, 0, 102, 102], [8, 9, 10, 11]])
    tok, lab = m.scst_inputs(seq)
    assert tok.shape == (2, 10) and (tok[:, 0] == m.bos_token).all() and (tok[:, 5:] == m.text_mask_token).all()
    assert tok[0, 1:5].tolist() == [7, 0, 102, 102]
    assert lab[0].tolist() == [-1] * 5 + [7, 0, 102, -1, -1] and lab[1].tolist() == [-1] * 5 + [8, 9, 10, 11, -1]
    m.caption_type = "lm"
    tok, lab = m.scst_inputs(seq)
    assert tok.shape == (2, 5) and lab[0].tolist() == [7, 0, 102, -1, -1]


def test_sampler_and_weighted_xent_validate_arguments_without_gpu():
    from valor_amd import lib
    so = lib.load()
    f = (ctypes.c_float * 64)()
    u8 = (ctypes.c_uint8 * 4)()
    i64 = (ctypes.c_int64 * 16)()

    def sample(R=4, V=16, ld=16, eos=3, logits=f, unf=u8, tok=i64, sents=i64, lp=f):
        return so.valor_sample_tokens(None, logits, ld, R, V, 1, 0, eos, unf, tok, sents, 1, lp, 1)
    assert sample(R=0) == -1 and sample(R=-1) == -1 and sample(V=0) == -1 and sample(ld=8) == -1
    assert sample(eos=16) == -1 and sample(eos=-1) == -1
    assert sample(logits=None) == -1 and sample(unf=None) == -1 and sample(tok=None) == -1 and sample(sents=None) == -1 and sample(lp=None) == -1
    assert so.valor_weighted_mean_f32(None, f, f, 0, f) == -1 and so.valor_weighted_mean_f32(None, f, None, 4, f) == -1
    assert so.valor_xent_weighted_bwd(None, 1, f, i64, f, f, None, 1.0, 0, 16, 16) == 0          # no rows: no-op
    assert so.valor_xent_weighted_bwd(None, 1, None, i64, f, f, None, 1.0, 4, 16, 16) == -1
    assert so.valor_xent_weighted_bwd(None, 7, f, i64, f, f, None, 1.0, 4, 16, 16) == -1          # unknown dtype
