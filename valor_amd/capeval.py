"""Corpus caption metrics of an evaluation run: Bleu_1..4, ROUGE_L and CIDEr of ONE hypothesis per clip against the clip's reference
captions -- what the reference's COCOEvalCap (cococaption/pycocoevalcap/eval.py) reports after tokenization, METEOR excepted (below).
CaptionMetrics is the host scorer (numpy / Python, in the style of scst.CaptionScorer, whose CIDEr it reuses); DeviceCaptionMetrics
computes the same numbers with valor_caption_metrics (csrc/capeval.hip) on symbol-id matrices that stay on the device, from the flat
tables capeval_tables builds; metrics_from_tables walks those tables in numpy (the table format checked without a GPU).

  * BLEU (bleu/bleu_scorer.py:201-266, called with option 'closest', bleu/bleu.py:43). Per clip: testlen, guess_k = max(0, testlen - k + 1),
    correct_k = sum over the hypothesis' k-grams of min(count, the maximum count in any one reference of the clip) (:63-86); the closest
    reference length, ties to the shorter (:74, :191). Corpus Bleu_k = (prod_{j <= k} (C_j + 1e-15) / (G_j + 1e-9))^(1/k) on the summed
    integers, times exp(1 - 1 / ratio) when ratio = (T + 1e-15) / (R + 1e-9) < 1 (:250-259). The per-clip values are the same formula on
    the clip's own integers (:234-242).
  * ROUGE-L (rouge/rouge.py:47-77): P = max_q lcs_q / len(hyp), R = max_q lcs_q / len(ref_q), the two maxima taken independently;
    score = (1 + b^2) P R / (R + b^2 P), b = 1.2, and 0 if either maximum is 0. An empty hypothesis scores 0 (the reference splits '' into
    one empty word that matches nothing). Corpus value: the mean over clips (:103).
  * CIDEr (cider/cider_scorer.py:96-195): the law of scst.CaptionScorer.cider (clipping, sigma 6, idf = ref_len - log(max(1, df))), with
    the document frequency and ref_len = log(#clips) counted over EXACTLY THE CLIPS BEING EVALUATED -- the ids of the results
    (eval.py:21, cider_scorer.py:103-106, :165) --, not over a fixed training list. Corpus value: the mean over clips (:195).

What is not reproduced. The reference pipes every caption through the Stanford PTB tokenizer and computes METEOR, both Java programs:
METEOR is left out (the dicts have the six other keys), and tokenization is a parameter: references and hypotheses are WORD LISTS (e.g.
PTB-tokenized captions cached elsewhere), or strings split by a `tokenize` callable, by default simple_tokenize below.

Symbols. Words are interned to small integers: reference words at construction (1, 2, ..), hypothesis words at call time (words in no
reference get the next free numbers for that call only); END = 0 is the end mark that pads the rows of an id matrix. Integer "words"
(model token ids) are taken as they are -- token-space metrics -- and the caller names the end mark (the model's [SEP])."""
import re
from collections import namedtuple

import numpy as np

from . import scst
from .scst import N, bleu_values, ngram_counts  # noqa: F401  (bleu_values: importable from here as before)

END = 0
BETA = 1.2
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
MAX_ROW_LEN = scst.MAX_ROW_LEN

# corpus: {key: float} (raw, not * 100); per_clip: {key: fp64 [R], 'correct' / 'guess': int [R, 4], 'testlen' / 'reflen': int [R]} in the
# order of `ids` (what COCOEvalCap keeps in videoToEval) or None; totals: the ten corpus integers {'correct': [4], 'guess': [4], 'testlen', 'reflen'}
CapEval = namedtuple("CapEval", "corpus per_clip totals")

_WORD = re.compile(r"[^\W_]+")


def simple_tokenize(caption):
    """caption string -> word list: lower-case, split on whitespace, punctuation split off the words, punctuation-only tokens dropped
    (so every run of letters / digits is a word). NOT the PTB tokenizer of the reference: PTB keeps clitics as tokens of their own
    ("man's" -> man 's, "don't" -> do n't; here man s, don t), rewrites brackets to -LRB- / -RRB- before dropping them and keeps a
    hyphenated word whole. For captions of plain words the two agree; feed PTB-tokenized word lists to reproduce the reference exactly."""
    return _WORD.findall(caption.lower())


def lcs_length(a, b):
    """length of the longest common subsequence of two sequences (rouge.py:15-36 computes the same number)"""
    if len(a) < len(b):
        a, b = b, a
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for j, y in enumerate(b):
            keep = row[j + 1]
            row[j + 1] = diag + 1 if x == y else max(keep, row[j])
            diag = keep
    return row[len(b)]


def rouge_l(hyp, refs):
    """rouge.py:47-77 on symbol lists"""
    if not hyp:
        return 0.0
    lcs = [lcs_length(r, hyp) for r in refs]
    prec = max(l / float(len(hyp)) for l in lcs)
    rec = max(l / float(max(len(r), 1)) for l, r in zip(lcs, refs))
    if prec != 0 and rec != 0:
        return ((1 + BETA ** 2) * prec * rec) / float(rec + BETA ** 2 * prec)
    return 0.0


def _assemble(cider, rouge, correct, guess, testlen, reflen, per_clip=True):
    """per-clip arrays -> CapEval"""
    correct, guess = np.asarray(correct, dtype=np.int64).reshape(-1, N), np.asarray(guess, dtype=np.int64).reshape(-1, N)
    testlen, reflen = np.asarray(testlen, dtype=np.int64), np.asarray(reflen, dtype=np.int64)
    bad = testlen < 0                                                          # rows without a score (the table walker / the device)
    totals = dict(correct=correct[~bad].sum(axis=0).tolist(), guess=guess[~bad].sum(axis=0).tolist(), testlen=int(testlen[~bad].sum()),
                  reflen=int(reflen[~bad].sum()))
    b = bleu_values(totals["correct"], totals["guess"], totals["testlen"], totals["reflen"])
    mean = lambda v: float(np.mean(v)) if len(v) else 0.0                     # no clip at all: zeros, as the device's summary
    corpus = dict(zip(KEYS, b + [mean(rouge), mean(cider)]))
    if bad.any():
        corpus = dict.fromkeys(KEYS, float("nan"))
    rows = None
    if per_clip:
        sent = np.array([[np.nan] * N if bad[i] else bleu_values(correct[i], guess[i], testlen[i], reflen[i]) for i in range(len(testlen))]).reshape(-1, N)
        rows = {f"Bleu_{k + 1}": sent[:, k] for k in range(N)}
        rows.update(ROUGE_L=np.asarray(rouge, dtype=np.float64), CIDEr=np.asarray(cider, dtype=np.float64), correct=correct, guess=guess,
                    testlen=testlen, reflen=reflen)
    return CapEval(corpus, rows, totals)


def rounded(corpus):
    """the reference's val_log entry (test.py:787): every value * 100, rounded to two decimals"""
    return {k: round(v * 100, 2) for k, v in corpus.items()}


class CaptionMetrics:
    """The host scorer. refs_by_id: {clip id: [word list, ...]} -- words are strings (interned here) or non-negative integers (model token
    ids, taken as they are); with `tokenize` the references may be caption strings.
      score(ids, hyps) -> CapEval(corpus, per_clip, totals): hyps[i] is the ONE hypothesis of clip ids[i] (a word list, or a string with
      `tokenize`). ValueError for a clip id that occurs twice (the reference asserts one hypothesis per clip, bleu.py:36) and for a clip
      without references, KeyError for an unknown clip id."""

    def __init__(self, refs_by_id, tokenize=None):
        self.tokenize = tokenize
        self.words = {}                                                        # word -> symbol (1, 2, ..); stays empty for integer words
        self.interned = None
        self.refs = {cid: [self._intern(self._words(r)) for r in refs] for cid, refs in refs_by_id.items()}
        if self.interned is None:
            self.interned = True
        self.n_symbols = len(self.words) + 1 if self.interned else 1 + max((t for refs in self.refs.values() for r in refs for t in r), default=0)
        self._stats = (None, None)

    @classmethod
    def from_annotations(cls, annfile, tokenize=simple_tokenize):
        """the reference's annotation file {'annotations': [{'video_id', 'caption'}, ...]} (every annotation is a reference)"""
        import json
        with open(annfile) as fh:
            anns = json.load(fh)["annotations"]
        refs = {}
        for a in anns:
            refs.setdefault(a["video_id"], []).append(a["caption"])
        return cls(refs, tokenize=tokenize)

    def _words(self, caption):
        if isinstance(caption, str):
            if self.tokenize is None:
                raise TypeError("CaptionMetrics: a caption string needs a `tokenize` callable (captions are word lists otherwise)")
            return self.tokenize(caption)
        return list(caption)

    def _intern(self, words, extra=None):
        """word list -> symbol list. Reference words (extra is None) enter self.words; a hypothesis word in no reference takes a number
        from `extra`, the overlay of one call"""
        out = []
        for w in words:
            is_str = isinstance(w, str)
            if self.interned is None:
                self.interned = is_str
            if is_str != self.interned:
                raise TypeError("CaptionMetrics: words are all strings or all integers (token ids), not a mixture")
            if not is_str:
                w = int(w)
                if w < 0:
                    raise ValueError(f"CaptionMetrics: the integer word {w} is negative")
                out.append(w)
                continue
            s = self.words.get(w)
            if s is None:
                if extra is None:
                    s = self.words[w] = len(self.words) + 1
                else:
                    s = extra.get(w)
                    if s is None:
                        s = extra[w] = self.n_symbols + len(extra)
            out.append(s)
        return out

    def encode(self, hyps):
        """hypotheses (word lists, or strings with `tokenize`) -> (symbol lists, the number of symbols in use: the references' and the
        new words of these hypotheses)"""
        extra = {}
        sym = [self._intern(self._words(h), extra) for h in hyps]
        if self.interned:
            return sym, self.n_symbols + len(extra)
        return sym, max(self.n_symbols, 1 + max((t for h in sym for t in h), default=0))

    def check_ids(self, ids, n_hyps=None):
        ids = list(ids)
        if n_hyps is not None and len(ids) != n_hyps:
            raise ValueError(f"CaptionMetrics: {len(ids)} ids for {n_hyps} hypotheses")
        seen = set()
        for i in ids:
            if i in seen:
                raise ValueError(f"CaptionMetrics: clip {i!r} occurs twice: the metrics take exactly one hypothesis per evaluated clip")
            seen.add(i)
            if not self.refs[i]:                                               # KeyError for an unknown clip
                raise ValueError(f"CaptionMetrics: clip {i!r} has no reference caption")
        return ids

    def stats(self, ids):
        """the n-gram statistics of the evaluated clips: a scst.CaptionScorer over exactly these clips, so that its document frequency
        and ref_len are those of cider_scorer.py:96-106, :165. Kept for the next call with the same clips."""
        key = frozenset(ids)
        if self._stats[0] != key:
            self._stats = (key, scst.CaptionScorer({i: self.refs[i] for i in ids}))
        return self._stats[1]

    def score(self, ids, hyps):
        ids = self.check_ids(ids, len(hyps))
        sym, _ = self.encode(hyps)
        st = self.stats(ids) if ids else None
        cider, rouge, correct, guess, testlen, reflen = [], [], [], [], [], []
        for cid, h in zip(ids, sym):
            cider.append(st.cider(cid, h))
            rouge.append(rouge_l(h, self.refs[cid]))
            reflens, maxc = st._bleu_refs[cid]
            correct.append(scst.clipped_counts((len(g) - 1, n, maxc.get(g, 0)) for g, n in ngram_counts(h).items()))
            guess.append(scst.guesses(len(h)))
            testlen.append(len(h))
            reflen.append(scst.closest_length(reflens, len(h)))
        return _assemble(cider, rouge, correct, guess, testlen, reflen)

    def to_device(self, device="cuda:0", eos=None, vocab=None):
        return DeviceCaptionMetrics(self, device=device, eos=eos, vocab=vocab)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The device scorer (valor_caption_metrics, csrc/capeval.hip): the statistics of the EVALUATED clips as the sorted key tables of the SCST
# reward (scst.reward_tables: the same n-gram keys, scst.pack_key with 16-bit fields) plus the references' raw symbols for the LCS.
def capeval_tables(metrics, ids):
    """CaptionMetrics, the evaluated clip ids -> the flat tables of valor_capeval_tables (include/valor_hip.h) as numpy arrays; clip c of
    the table is ids[c] ('clips'). Every float comes from the host statistics. ValueError when a symbol does not fit the 16-bit key fields."""
    ids = metrics.check_ids(ids)
    top = max((t for i in ids for r in metrics.refs[i] for t in r), default=0)
    if top > scst.MAX_TOKEN:
        raise ValueError(f"capeval_tables: the references use symbols up to {top}; the device keys hold 0..{scst.MAX_TOKEN} (16-bit fields). "
                         "CaptionMetrics is the host scorer")
    st = metrics.stats(ids)
    if list(st.refs) != ids:                                                   # the cached statistics may list the clips in another order
        st = scst.CaptionScorer({i: metrics.refs[i] for i in ids})
    T = scst.reward_tables(st)
    flat = [r for i in ids for r in metrics.refs[i]]
    T["ref_sym_ptr"] = np.cumsum([0] + [len(r) for r in flat]).astype(np.int32)
    T["ref_syms"] = np.array([t for r in flat for t in r], dtype=np.uint16)
    return T


def _bit_lcs(hyp, ref):
    """the kernel's bit-parallel LCS on a Python integer: V = (V + (V & M)) | (V & ~M) per reference symbol, LCS = the zero bits of V"""
    full = (1 << len(hyp)) - 1
    masks = {}
    for j, w in enumerate(hyp):
        masks[w] = masks.get(w, 0) | (1 << j)
    v = full
    for s in ref:
        m = masks.get(s, 0)
        v = ((v + (v & m)) | (v & ~m)) & full
    return len(hyp) - bin(v).count("1")


def metrics_from_tables(tables, clip_idx, seqs, eos, vocab=scst.MAX_VOCAB, per_clip=True):
    """The walk valor_caption_metrics does, in numpy on the flat tables: seqs int [R, L] (or rows of different lengths), clip_idx [R] ->
    CapEval. A row is cut at its first `eos`; a symbol outside [0, vocab) matches nothing; a row of a clip without references has NaN
    values and -1 integers, and makes every corpus value NaN."""
    T = tables
    cider, rouge, correct, guess, testlen, reflen = [], [], [], [], [], []
    for hyp, (ref0, ref1), cid, cc, rl in scst.walk_rows(T, clip_idx, seqs, eos, vocab):          # CIDEr and BLEU's integers are the reward's
        if cc is None:
            cider.append(np.nan), rouge.append(np.nan), correct.append([-1] * N), guess.append([-1] * N), testlen.append(-1), reflen.append(-1)
            continue
        cider.append(cid), correct.append(cc), guess.append(scst.guesses(len(hyp))), testlen.append(len(hyp)), reflen.append(rl)
        best, rec = 0, 0.0
        inside = [t if 0 <= t < vocab else None for t in hyp]
        for q in range(ref0, ref1):
            ref = T["ref_syms"][int(T["ref_sym_ptr"][q]):int(T["ref_sym_ptr"][q + 1])].tolist()
            l = _bit_lcs(inside, ref)
            best = max(best, l)
            if ref:
                rec = max(rec, l / float(len(ref)))
        prec = best / float(len(hyp)) if hyp else 0.0
        rouge.append(((1 + BETA ** 2) * prec * rec) / float(rec + BETA ** 2 * prec) if prec != 0 and rec != 0 else 0.0)
    return _assemble(cider, rouge, correct, guess, testlen, reflen, per_clip)


def upload_tables(T, dev):
    """scst.upload_tables for the tables of capeval_tables: (device tensors by field, a lib.CapevalTables of their addresses)"""
    from . import lib
    return scst.upload_tables(T, lib.CapevalTables, dev)


class DeviceCaptionMetrics:
    """CaptionMetrics computed by valor_caption_metrics. metrics_or_refs: a CaptionMetrics, or what its constructor takes. eos: the end
    mark of an id matrix (default END for interned words; required for integer words: the model's [SEP]). vocab: symbols outside
    [0, vocab) match nothing (id matrices only; default: every id a key can carry).
      score(ids, hyps, per_clip=False) -> CapEval. hyps: the hypotheses as CaptionMetrics.score takes them (they are interned, padded
      with the end mark and uploaded: one small id matrix), or an int64 [R, L] id matrix ON THE DEVICE (L <= MAX_ROW_LEN, rows cut at the
      first end mark, unit column stride, any row pitch), row i belonging to clip ids[i]. Only the summary (six values, ten totals) comes
      back to the host unless per_clip is asked for.
    The tables are built for the evaluated clip set `ids` and kept for the next call with the same ids -- the whole validation set on
    every validation round: one build, one upload. ValueError for duplicate / reference-less clips, for a vocabulary or a hypothesis
    that does not fit the device format (CaptionMetrics is the host scorer); KeyError for an unknown clip."""

    def __init__(self, metrics_or_refs, tokenize=None, device="cuda:0", eos=None, vocab=None):
        self.host = metrics_or_refs if isinstance(metrics_or_refs, CaptionMetrics) else CaptionMetrics(metrics_or_refs, tokenize=tokenize)
        if eos is None:
            if not self.host.interned:
                raise ValueError("DeviceCaptionMetrics: integer words (token ids) need the end mark `eos` of their id matrices")
            eos = END
        self.eos = int(eos)
        self.vocab = None if vocab is None else int(vocab)
        self.device = device
        self._tables = (None, None)          # (ids, numpy tables)
        self._dev = None                     # (ids, device, tensors, struct, clip_idx)

    def tables_for(self, ids):
        ids = list(ids)
        if self._tables[0] != ids:
            self._tables = (ids, capeval_tables(self.host, ids))
        return self._tables[1]

    def check(self, vocab, L=None):
        if not 1 <= vocab <= scst.MAX_VOCAB:
            raise ValueError(f"DeviceCaptionMetrics: {vocab} symbols (reference words plus new hypothesis words) do not fit the 16-bit key "
                             f"fields (1..{scst.MAX_VOCAB}); CaptionMetrics is the host scorer")
        if not 0 <= self.eos < vocab:
            raise ValueError(f"DeviceCaptionMetrics: the end mark {self.eos} is outside the vocabulary [0, {vocab})")
        if L is not None and not 1 <= L <= MAX_ROW_LEN:
            raise ValueError(f"DeviceCaptionMetrics: rows of {L} symbols; valor_caption_metrics takes 1..{MAX_ROW_LEN} (CaptionMetrics is the host scorer)")
        return vocab

    def id_matrix(self, hyps):
        """hypotheses -> (numpy int64 [R, L] padded with the end mark, the vocabulary in use)"""
        sym, vocab = self.host.encode(hyps)
        L = max([len(h) for h in sym] + [1])
        self.check(vocab, L)
        m = np.full((len(sym), L), self.eos, dtype=np.int64)
        for r, h in enumerate(sym):
            if self.eos in h:
                raise ValueError(f"DeviceCaptionMetrics: hypothesis {r} contains the end mark {self.eos}")
            m[r, :len(h)] = h
        return m, vocab

    def _upload(self, ids):
        import torch
        dev = torch.device(self.device)
        keep, st = upload_tables(self.tables_for(ids), dev)
        clip_idx = torch.arange(len(ids), dtype=torch.int32, device=dev)          # clip c of the table is ids[c]
        self._dev = (list(ids), dev, keep, st, clip_idx)
        return self._dev

    def score(self, ids, hyps, per_clip=False):
        import torch
        from . import kernels as K
        ids = list(ids)
        if not ids:
            return _assemble([], [], [], [], [], [], per_clip)
        if self._dev is None or self._dev[0] != ids:
            self.host.check_ids(ids)
            self._upload(ids)
        _, dev, _, st, clip_idx = self._dev
        if isinstance(hyps, torch.Tensor):
            seq = hyps
            vocab = self.check(scst.MAX_VOCAB if self.vocab is None else self.vocab, seq.shape[1] if seq.dim() == 2 else None)
        else:
            if len(hyps) != len(ids):
                raise ValueError(f"DeviceCaptionMetrics: {len(ids)} ids for {len(hyps)} hypotheses")
            m, vocab = self.id_matrix(hyps)
            seq = torch.from_numpy(m).to(dev)
        if seq.dim() != 2 or seq.shape[0] != len(ids):
            raise ValueError(f"DeviceCaptionMetrics: {len(ids)} ids for an id matrix of shape {tuple(seq.shape)}")
        R = seq.shape[0]
        f64 = torch.empty((6, R), dtype=torch.float64, device=dev)               # cider, rouge, bleu [R, 4]
        counts = torch.empty((R, 10), dtype=torch.int32, device=dev)
        summary = torch.empty((16,), dtype=torch.int64, device=dev)
        K.caption_metrics(seq, self.eos, vocab, clip_idx, st, f64[0], f64[1], f64[2:].view(-1), counts, summary)
        s = summary.cpu()
        value, total = s[:6].view(torch.float64).tolist(), s[6:].tolist()
        totals = dict(correct=total[:4], guess=total[4:8], testlen=total[8], reflen=total[9])
        rows = None
        if per_clip:
            f, c = f64.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
            b = f[2:].reshape(R, N)
            rows = {f"Bleu_{k + 1}": b[:, k].copy() for k in range(N)}
            rows.update(ROUGE_L=f[1].copy(), CIDEr=f[0].copy(), correct=c[:, :4], guess=c[:, 4:8], testlen=c[:, 8], reflen=c[:, 9])
        return CapEval(dict(zip(KEYS, value)), rows, totals)
