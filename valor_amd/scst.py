"""The caption reward of self-critical sequence training (SCST): CIDEr-D + BLEU-4 per hypothesis, weights [1, 1] -- what the reference's
`Scorer` (scorer/scorer.py:31-80) computes on token-id lists, written for the training loop: every reference caption's n-gram
statistics (CIDEr-D tf-idf vectors and norms, BLEU maximum counts and lengths) are computed ONCE at construction, a call only cooks the
hypotheses. Host-side numpy / Python: the scorer is the reference's host code too. DeviceCaptionScorer (below) is the same reward on the
device: the statistics flattened into sorted n-gram key tables, scored by valor_caption_reward (csrc/reward.hip) on id matrices that stay
there; walk_rows / reward_from_tables walk those tables in numpy.

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


def clipped_counts(grams):
    """BLEU's correct_k, k = 1..4, from (n - 1, the hypothesis' count, the clip's maximum count in one reference) per distinct n-gram"""
    correct = [0] * N
    for n, c, m in grams:
        correct[n] += min(m, c)
    return correct


def guesses(testlen):
    """BLEU's guess_k = the number of k-grams of a hypothesis of `testlen` tokens"""
    return [max(0, testlen - k) for k in range(N)]


def closest_length(reflens, testlen):
    """the reference length closest to testlen, ties to the shorter (bleu_scorer.py 'closest')"""
    return min((abs(int(l) - testlen), int(l)) for l in reflens)[1]


def bleu_values(correct, guess, testlen, reflen):
    """bleu_scorer.py:234-242 / :250-259: Bleu_1..4 from one set of integers (a clip's, or the corpus totals)"""
    out = []
    b = 1.0
    for k in range(N):
        b *= (float(correct[k]) + _TINY) / (float(guess[k]) + _SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + _TINY) / (reflen + _SMALL)
    if ratio < 1:
        out = [v * np.exp(1 - 1 / ratio) for v in out]
    return [float(v) for v in out]


def _bleu4(correct, testlen, reflen):
    """the reward's sentence BLEU-4. bleu_values(..)[3] up to the last bit of its brevity penalty: math.exp here, np.exp there, and the
    two differ by an ulp on some ratios, so the reward keeps its own"""
    b = 1.0
    for k in range(N):
        b *= (float(correct[k]) + _TINY) / (float(max(0, testlen - k)) + _SMALL)
    b = b ** (1.0 / N)
    ratio = (testlen + _TINY) / (reflen + _SMALL)
    if ratio < 1:
        b *= math.exp(1 - 1 / ratio)
    return b


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
        correct = clipped_counts((len(g) - 1, c, maxc.get(g, 0)) for g, c in ngram_counts(hyp).items())
        return _bleu4(correct, len(hyp), closest_length(reflens, len(hyp)))

    def __call__(self, ids, hyps):
        if len(ids) != len(hyps):
            raise ValueError(f"CaptionScorer: {len(ids)} ids for {len(hyps)} hypotheses")
        out = np.zeros(len(hyps))
        for i, (cid, h) in enumerate(zip(ids, hyps)):
            h = [int(x) for x in h]
            out[i] += self.cider(cid, h)
            out[i] += self.bleu4(cid, h)
        return out

    def to_device(self, device="cuda:0", vocab=None):
        """the same reward computed on the device (DeviceCaptionScorer) from this scorer's statistics"""
        return DeviceCaptionScorer(self, device=device, vocab=vocab)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The device scorer (valor_caption_reward, csrc/reward.hip): the statistics above flattened into sorted arrays of 64-bit n-gram keys.
#   key of (t_0 .. t_{n-1}) = sum (t_i + 1) << 16 i: exact and collision-free for token ids 0 .. 65533 (BERT: 30 522 entries, CLIP: 49 408),
#   n = the number of non-zero 16-bit fields. Code 65535 is "unknown": a hypothesis token outside the vocabulary; no table key carries it.
MAX_TOKEN = 65533
MAX_VOCAB = MAX_TOKEN + 1
UNKNOWN = 65535
MAX_ROW_LEN = 128                    # valor_caption_reward's limit on L


def pack_key(gram):
    """n-gram (1 <= n <= 4 token ids in 0 .. MAX_TOKEN) -> its key (Python int below 2^64)"""
    if not 1 <= len(gram) <= N:
        raise ValueError(f"pack_key: an n-gram has 1..{N} tokens, not {len(gram)}")
    key = 0
    for i, t in enumerate(gram):
        t = int(t)
        if not 0 <= t <= MAX_TOKEN:
            raise ValueError(f"pack_key: token id {t} outside 0..{MAX_TOKEN} (16-bit key fields; {UNKNOWN} is the unknown code)")
        key |= (t + 1) << (16 * i)
    return key


def unpack_key(key):
    """key -> n-gram tuple"""
    key = int(key)
    out = []
    while key:
        out.append((key & 0xFFFF) - 1)
        key >>= 16
    return tuple(out)


def reward_tables(scorer):
    """CaptionScorer -> the flat tables of valor_reward_tables (include/valor_hip.h) as numpy arrays, plus 'clips' (the clip ids in
    table order). Every float is taken from the scorer (or evaluated with its expression): the device works on the host's bits.
    Raises ValueError for a reference token outside 0 .. MAX_TOKEN."""
    for cid, refs in scorer.refs.items():
        for r in refs:
            for t in r:
                if not 0 <= t <= MAX_TOKEN:
                    raise ValueError(f"reward_tables: clip {cid!r} has the reference token {t}, outside 0..{MAX_TOKEN}")
    g = sorted((pack_key(gram), df) for gram, df in scorer.df.items())
    g_keys = np.array([k for k, _ in g], dtype=np.uint64)
    g_idf = np.array([scorer.ref_len - np.log(max(1.0, df)) for _, df in g], dtype=np.float64)          # CaptionScorer._vec's expression
    clips = list(scorer.refs)
    clip_ref_ptr, ref_key_ptr, clip_bleu_ptr = [0], [0], [0]
    ref_keys, ref_vals, ref_norm, ref_bigrams, ref_tokens, bleu_keys, bleu_cnt = [], [], [], [], [], [], []
    for cid in clips:
        for (vec, norm, length), r in zip(scorer._cider_refs[cid], scorer.refs[cid]):
            kv = sorted((pack_key(gram), v) for d in vec for gram, v in d.items())
            ref_keys += [k for k, _ in kv]
            ref_vals += [v for _, v in kv]
            ref_key_ptr.append(len(ref_keys))
            ref_norm.append([float(x) for x in norm])
            ref_bigrams.append(int(length))
            ref_tokens.append(len(r))
        clip_ref_ptr.append(len(ref_tokens))
        kc = sorted((pack_key(gram), c) for gram, c in scorer._bleu_refs[cid][1].items())
        bleu_keys += [k for k, _ in kc]
        bleu_cnt += [c for _, c in kc]
        clip_bleu_ptr.append(len(bleu_keys))
    if max(len(ref_keys), len(bleu_keys), len(g)) >= 2 ** 31:
        raise ValueError("reward_tables: more than 2^31 table entries (int32 offsets)")
    i32 = lambda a: np.array(a, dtype=np.int32)
    return dict(g_keys=g_keys, g_idf=g_idf, ref_len=float(scorer.ref_len), clip_ref_ptr=i32(clip_ref_ptr), ref_key_ptr=i32(ref_key_ptr),
                ref_keys=np.array(ref_keys, dtype=np.uint64), ref_vals=np.array(ref_vals, dtype=np.float64),
                ref_norm=np.array(ref_norm, dtype=np.float64).reshape(-1, N), ref_bigrams=i32(ref_bigrams), ref_tokens=i32(ref_tokens),
                clip_bleu_ptr=i32(clip_bleu_ptr), bleu_keys=np.array(bleu_keys, dtype=np.uint64), bleu_cnt=i32(bleu_cnt), clips=clips)


def _find(keys, lo, hi, key):
    j = lo + int(np.searchsorted(keys[lo:hi], np.uint64(key)))
    return j if j < hi and int(keys[j]) == key else -1


def walk_rows(tables, clip_idx, seqs, eos, vocab=MAX_VOCAB):
    """The walk the device kernels do, in numpy on the flat tables (the table format checked without a GPU): seqs int [R, L] (or rows of
    different lengths), clip_idx [R] -> per row (hyp, (ref0, ref1), CIDEr, correct[4], reflen). A row is cut at its first `eos`: hyp, of
    len(hyp) tokens; a token outside [0, vocab) takes the unknown code and matches nothing; a row of a clip without references
    (ref1 <= ref0) has None for its three values."""
    T = tables
    rows = seqs.tolist() if hasattr(seqs, "tolist") else [list(r) for r in seqs]
    for r, row in enumerate(rows):
        row = [int(x) for x in row]
        hyp = row[:row.index(eos)] if eos in row else row
        c = int(clip_idx[r])
        ref0, ref1 = (int(T["clip_ref_ptr"][c]), int(T["clip_ref_ptr"][c + 1])) if 0 <= c < len(T["clip_ref_ptr"]) - 1 else (0, 0)
        if ref1 <= ref0:
            yield hyp, (0, 0), None, None, None
            continue
        # (n, key, tf, x): counted on the raw tokens, so two different unknown tokens stay two n-grams
        grams = []
        for gram, tf in ngram_counts(hyp).items():
            key = 0
            for i, t in enumerate(gram):
                key |= ((t + 1) if 0 <= t < vocab else UNKNOWN) << (16 * i)
            j = _find(T["g_keys"], 0, len(T["g_keys"]), key)
            grams.append((len(gram) - 1, key, tf, float(tf) * (T["g_idf"][j] if j >= 0 else T["ref_len"])))
        norm = [0.0] * N
        for n, _, _, x in grams:
            norm[n] += x * x
        norm = np.sqrt(norm)
        lh = max(len(hyp) - 1, 0)
        score = np.zeros(N)
        for q in range(ref0, ref1):
            lo, hi = int(T["ref_key_ptr"][q]), int(T["ref_key_ptr"][q + 1])
            val = np.zeros(N)
            for n, key, _, x in grams:
                j = _find(T["ref_keys"], lo, hi, key)
                if j >= 0:
                    y = T["ref_vals"][j]
                    val[n] += min(x, y) * y
            delta = float(lh - int(T["ref_bigrams"][q]))
            for n in range(N):
                if norm[n] != 0 and T["ref_norm"][q, n] != 0:
                    val[n] /= norm[n] * T["ref_norm"][q, n]
            score += val * math.exp(-(delta * delta) / (2 * SIGMA ** 2))
        b0, b1 = int(T["clip_bleu_ptr"][c]), int(T["clip_bleu_ptr"][c + 1])
        found = ((n, tf, _find(T["bleu_keys"], b0, b1, key)) for n, key, tf, _ in grams)
        correct = clipped_counts((n, tf, int(T["bleu_cnt"][j]) if j >= 0 else 0) for n, tf, j in found)
        yield hyp, (ref0, ref1), score.sum() / N / (ref1 - ref0) * 10.0, correct, closest_length(T["ref_tokens"][ref0:ref1], len(hyp))


def reward_from_tables(tables, clip_idx, seqs, eos, vocab=MAX_VOCAB, parts=False):
    """What valor_caption_reward returns, from walk_rows: fp64 reward [R] (parts: (reward, CIDEr-D, BLEU-4)); NaN for a row of a clip
    without references."""
    walk = list(walk_rows(tables, clip_idx, seqs, eos, vocab))
    cider, bleu = np.zeros(len(walk)), np.zeros(len(walk))
    for r, (hyp, _, cid, correct, reflen) in enumerate(walk):
        cider[r], bleu[r] = (np.nan, np.nan) if correct is None else (cid, _bleu4(correct, len(hyp), reflen))
    return (cider + bleu, cider, bleu) if parts else cider + bleu


def upload_tables(T, struct_cls, dev):
    """the numpy tables of reward_tables / capeval.capeval_tables -> (device tensors by field, a struct_cls (lib.RewardTables,
    lib.CapevalTables) of their addresses); keep the tensors alive as long as the struct is used"""
    import torch
    from . import lib
    if dev.type != "cuda":
        raise lib.ValorHipError("the device caption scorers score on the GPU (no CPU fallback); CaptionScorer / CaptionMetrics are the host scorers")
    st = struct_cls()
    keep = {}
    for k in struct_cls.POINTERS:
        a = T[k]
        if a.size == 0:                                   # an empty list still gets an address
            a = np.zeros(1, dtype=a.dtype)
        a = np.ascontiguousarray(a)
        view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}.get(a.dtype)          # torch has no unsigned of these widths
        keep[k] = torch.from_numpy(a.view(view) if view else a).to(dev)
        setattr(st, k, keep[k].data_ptr())
    st.ref_len = T["ref_len"]
    st.n_global = int(T["g_keys"].size)
    st.n_clips = len(T["clips"])
    return keep, st


class DeviceCaptionScorer:
    """The reward of CaptionScorer computed by valor_caption_reward on token-id matrices that stay on the device.
    scorer_or_refs: a CaptionScorer, or {clip id: [token-id list, ...]} with df_ids as CaptionScorer takes them. vocab: hypothesis tokens
    outside [0, vocab) match nothing (default: every id a key can carry). The tables are built here (ValueError for a reference token
    above MAX_TOKEN) and uploaded at the first call.
      score(ids, seq, eos) -> fp64 [R] on the device: seq int64 [R, L] device tensor (L <= MAX_ROW_LEN, unit column stride), ids the R
        clip ids, or their int32 table indices as clip_index gives them (unchecked: a row whose index is outside the table, or whose
        clip has no reference, scores NaN). ValueError for what check() names.
      advantages(ids, samples, baselines, eos) -> per group the fp32 [b] tensor reward(sample) - reward(baseline), one launch in all"""

    def __init__(self, scorer_or_refs, df_ids=None, device="cuda:0", vocab=None):
        if isinstance(scorer_or_refs, CaptionScorer):
            if df_ids is not None:
                raise ValueError("DeviceCaptionScorer: df_ids belongs to the CaptionScorer it is built from")
            self.host = scorer_or_refs
        else:
            self.host = CaptionScorer(scorer_or_refs, df_ids=df_ids)
        self.tables = reward_tables(self.host)
        self.clip_of = {cid: i for i, cid in enumerate(self.tables["clips"])}
        self.vocab = MAX_VOCAB if vocab is None else int(vocab)
        self.device = device
        self._dev = None

    def clip_index(self, ids):
        """clip ids -> int32 table indices; KeyError for an unknown id (as the host scorer), ValueError for a clip without references"""
        idx = np.array([self.clip_of[i] for i in ids], dtype=np.int32)
        ptr = self.tables["clip_ref_ptr"]
        for i, c in zip(ids, idx):
            if ptr[c + 1] == ptr[c]:
                raise ValueError(f"DeviceCaptionScorer: clip {i!r} has no reference caption")
        return idx

    def check(self, eos, vocab=None, L=None):
        """ValueError for a geometry valor_caption_reward does not take: vocab outside 1..MAX_VOCAB, eos outside [0, vocab), rows wider
        than MAX_ROW_LEN. -> the vocabulary in use"""
        vocab = self.vocab if vocab is None else int(vocab)
        if not 1 <= vocab <= MAX_VOCAB:
            raise ValueError(f"DeviceCaptionScorer: a vocabulary of {vocab} entries does not fit the 16-bit key fields (1..{MAX_VOCAB}); "
                             "CaptionScorer is the host scorer")
        if not 0 <= int(eos) < vocab:
            raise ValueError(f"DeviceCaptionScorer: eos = {int(eos)} is outside the vocabulary [0, {vocab})")
        if L is not None and not 1 <= L <= MAX_ROW_LEN:
            raise ValueError(f"DeviceCaptionScorer: rows of {L} tokens; valor_caption_reward takes 1..{MAX_ROW_LEN}")
        return vocab

    def _upload(self):
        import torch
        from . import lib
        dev = torch.device(self.device)
        self._dev = (dev,) + upload_tables(self.tables, lib.RewardTables, dev)
        return self._dev

    def score(self, ids, seq, eos, vocab=None, parts=False):
        import torch
        from . import kernels as K
        dev, _, st = self._dev or self._upload()
        idx = ids if isinstance(ids, np.ndarray) and ids.dtype == np.int32 else self.clip_index(ids)
        if seq.dim() != 2 or idx.shape[0] != seq.shape[0]:
            raise ValueError(f"DeviceCaptionScorer: {idx.shape[0]} ids for sequences of shape {tuple(seq.shape)}")
        vocab = self.check(eos, vocab, seq.shape[1])
        clip_idx = torch.from_numpy(idx).to(dev)
        R = seq.shape[0]
        out = torch.empty((3 if parts else 1, R), dtype=torch.float64, device=dev)
        K.caption_reward(seq, int(eos), vocab, clip_idx, st, out[0], out[1] if parts else None, out[2] if parts else None)
        return (out[0], out[1], out[2]) if parts else out[0]

    def advantages(self, ids, samples, baselines, eos, vocab=None):
        import torch
        if len(samples) != len(baselines):
            raise ValueError("DeviceCaptionScorer: one baseline matrix per sample matrix")
        idx = self.clip_index(ids)
        rows = list(samples) + list(baselines)
        width = max(t.shape[1] for t in rows)
        if any(t.shape[1] != width for t in rows):        # a shorter matrix is padded with eos: nothing behind the cut counts
            rows = [torch.nn.functional.pad(t, (0, width - t.shape[1]), value=int(eos)) for t in rows]
        rw = self.score(np.tile(idx, len(rows)), torch.cat(rows, dim=0), eos, vocab)
        n = rw.shape[0] // 2
        adv = (rw[:n] - rw[n:]).to(torch.float32)         # fp64 difference, then one rounding: the host path's order
        return list(adv.split(len(idx)))
