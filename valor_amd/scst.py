"""The caption reward of self-critical sequence training (SCST): CIDEr-D + BLEU-4 per hypothesis, weights [1, 1] -- what the reference's
`Scorer` (scorer/scorer.py:31-80) computes on token-id lists, written for the training loop: every reference caption's n-gram
statistics (CIDEr-D tf-idf vectors and norms, BLEU maximum counts and lengths) are computed ONCE at construction, a call only cooks the
hypotheses. Host-side numpy / Python: the scorer is the reference's host code too.

  * CIDEr-D (scorer/cider_scorer.py:119-200): n = 1..4, sigma = 6; idf = ref_len - log(max(1, df)) with df counted over the clips of
    `df_ids` and ref_len = log(#those clips) (precompute_df_reflen_for_cider, scorer/scorer.py:117-147); per n the clipped dot product
    sum min(h, r) * r over the hypothesis' n-grams, divided by both norms when neither is 0, times the Gaussian length penalty
    exp(-delta^2 / (2 sigma^2)). The length is the BIGRAM count of a caption (the reference's counts2vec counts n == 1, the 2-grams: a
    quirk, kept). Score = mean over n, summed over the references, / #references, * 10.
  * BLEU-4 (scorer/bleu_scorer.py:202-250, option 'closest'): per sentence, prod_k (correct_k + 1e-15) / (guess_k + 1e-9), k = 1..4, to
    the power 1/4; times exp(1 - 1 / ratio) when ratio = (len + 1e-15) / (closest reference length + 1e-9) < 1.

Hypotheses are token-id lists cut at their first [SEP] (process_scst, model/pretrain.py:728-739: `hypotheses`)."""
import json
import math
from collections import defaultdict

import numpy as np

N = 4
SIGMA = 6.0
_TINY, _SMALL = 1e-15, 1e-9


def ngram_counts(words, n=N):
    """{n-gram tuple: count} for n = 1..n"""
    counts = defaultdict(int)
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            counts[tuple(words[i:i + k])] += 1
    return counts


def document_frequency(refs_by_id, ids):
    """(df, ref_len): per n-gram the number of clips of `ids` (that have references) whose references contain it, and log(#clips)"""
    df = defaultdict(int)
    clips = 0
    for i in ids:
        refs = refs_by_id.get(i)
        if not refs:
            continue
        clips += 1
        seen = set()
        for r in refs:
            seen.update(ngram_counts(r))
        for g in seen:
            df[g] += 1
    return df, float(np.log(float(clips)))


def hypotheses(seq, eos):
    """int [b, L] (tensor or array) -> token-id lists cut at the first `eos` (process_scst)"""
    rows = seq.tolist() if hasattr(seq, "tolist") else [list(r) for r in seq]
    out = []
    for r in rows:
        cut = r.index(eos) if eos in r else len(r)
        out.append([int(x) for x in r[:cut]])
    return out


class CaptionScorer:
    """scorer(ids, hyps) -> numpy float64 [len(hyps)]: CIDEr-D + BLEU-4 of hyps[i] against the reference captions of clip ids[i].
    refs_by_id: {clip id: [token-id list, ...]} (the model tokenizer's ids without [CLS] / [SEP], as tokenizer.encode gives them);
    df_ids: the clips the CIDEr document frequency is counted over (None: all of refs_by_id)."""

    def __init__(self, refs_by_id, df_ids=None):
        self.refs = {k: [list(map(int, r)) for r in v] for k, v in refs_by_id.items()}
        self.df, self.ref_len = document_frequency(self.refs, list(self.refs) if df_ids is None else list(df_ids))
        self._cider_refs = {}
        self._bleu_refs = {}
        for k, refs in self.refs.items():
            self._cider_refs[k] = [self._vec(ngram_counts(r)) for r in refs]
            maxc = {}
            for r in refs:
                for g, c in ngram_counts(r).items():
                    if c > maxc.get(g, 0):
                        maxc[g] = c
            self._bleu_refs[k] = ([len(r) for r in refs], maxc)

    @classmethod
    def from_annotations(cls, annfile, idsfile, encode):
        """the reference's files: annfile = {'annotations': [{'video_id', 'caption'}, ...]} (every annotation is a reference, preprocess_gts
        scorer/scorer.py:21-28), idsfile = a JSON list of clip ids (the clips df is counted over); encode: caption string -> token ids"""
        with open(annfile) as fh:
            anns = json.load(fh)["annotations"]
        with open(idsfile) as fh:
            ids = json.load(fh)
        refs = defaultdict(list)
        for a in anns:
            refs[a["video_id"]].append(list(encode(a["caption"])))
        return cls(dict(refs), df_ids=ids)

    def _vec(self, counts):
        vec = [dict() for _ in range(N)]
        norm = [0.0] * N
        length = 0
        for g, tf in counts.items():
            n = len(g) - 1
            v = float(tf) * (self.ref_len - np.log(max(1.0, self.df.get(g, 0))))
            vec[n][g] = v
            norm[n] += pow(v, 2)
            if n == 1:
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    def cider(self, cid, hyp):
        vh, nh, lh = self._vec(ngram_counts(hyp))
        refs = self._cider_refs[cid]
        score = np.zeros(N)
        for vr, nr, lr in refs:
            delta = float(lh - lr)
            val = np.zeros(N)
            for n in range(N):
                rn = vr[n]
                for g, x in vh[n].items():
                    y = rn.get(g, 0.0)
                    val[n] += min(x, y) * y
                if nh[n] != 0 and nr[n] != 0:
                    val[n] /= nh[n] * nr[n]
                val[n] *= np.e ** (-(delta ** 2) / (2 * SIGMA ** 2))
            score += val
        s = np.mean(score)
        s /= len(refs)
        return s * 10.0

    def bleu4(self, cid, hyp):
        reflens, maxc = self._bleu_refs[cid]
        testlen = len(hyp)
        reflen = min((abs(l - testlen), l) for l in reflens)[1]
        correct = [0] * N
        for g, c in ngram_counts(hyp).items():
            correct[len(g) - 1] += min(maxc.get(g, 0), c)
        b = 1.0
        for k in range(N):
            b *= (float(correct[k]) + _TINY) / (float(max(0, testlen - k)) + _SMALL)
        b = b ** (1.0 / N)
        ratio = (testlen + _TINY) / (reflen + _SMALL)
        if ratio < 1:
            b *= math.exp(1 - 1 / ratio)
        return b

    def __call__(self, ids, hyps):
        if len(ids) != len(hyps):
            raise ValueError(f"CaptionScorer: {len(ids)} ids for {len(hyps)} hypotheses")
        out = np.zeros(len(hyps))
        for i, (cid, h) in enumerate(zip(ids, hyps)):
            h = [int(x) for x in h]
            out[i] += self.cider(cid, h)
            out[i] += self.bleu4(cid, h)
        return out
