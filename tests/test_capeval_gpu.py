"""The caption evaluation metrics on the GPU (valor_caption_metrics, csrc/capeval.hip, through capeval.DeviceCaptionMetrics): per-clip
Bleu_1..4, ROUGE-L, CIDEr, their integers and the corpus summary against the unmodified reference's recorded values
(tests/golden/cap_metrics.pt) and against the host CaptionMetrics at the boundary lengths of the bit-parallel LCS (hypotheses of 0, 1, 63,
64, 65, 127, 128 symbols against references of 1, 64, 65, 200 symbols), for a clip with more references than the workgroup has lanes and
more n-gram entries than the LDS stage holds, and for R = 1, 257, 2990 rows of the corpus reduction; determinism and a strided id
matrix; NaN rows and the refused geometries; validate_cap / validate_qa end to end on the small synthetic model, on one process and on
two gloo ranks with unequal shards.

Tolerance of the fp64 comparisons: rtol 1e-9, atol 1e-12 (tests/test_reward_cpu.py's docstring: reordered sums of at most a few thousand
non-negative terms move by ~1e-13 relative, exp / sqrt / pow by a few ulp). Integers are compared exactly. No row is excluded."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_capeval_goldens import KEYS, load  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
INTS = ("correct", "guess", "testlen", "reflen")
EOS = 102


def _compare(tag, got, want):
    """device CapEval against a host CapEval: integers exact, fp64 per clip and corpus within the tolerance; every figure printed first"""
    for k in KEYS:
        g, w = np.asarray(got.per_clip[k]), np.asarray(want.per_clip[k])
        err = np.abs(g - w)
        print(f"[capeval {tag}] {k}: rows {g.size}, max |d| = {err.max() if g.size else 0:.3g}, corpus {got.corpus[k]!r} vs {want.corpus[k]!r}")
    for k in INTS:
        assert np.array_equal(got.per_clip[k], want.per_clip[k]), k
    assert got.totals == want.totals
    for k in KEYS:
        np.testing.assert_allclose(got.per_clip[k], want.per_clip[k], rtol=RTOL, atol=ATOL, err_msg=k)
        np.testing.assert_allclose(got.corpus[k], want.corpus[k], rtol=RTOL, atol=ATOL, err_msg=k)


def _pad(hyps, L, rng, eos=EOS, lo=1000, hi=1006):
    """int64 [R, L]: every hypothesis, its end mark, then symbols that would score if they were counted"""
    m = rng.integers(lo, hi, size=(len(hyps), L)).astype(np.int64)
    for r, h in enumerate(hyps):
        m[r, :len(h)] = h
        if len(h) < L:
            m[r, len(h)] = eos
    return m


def test_device_matches_the_reference_fixture(dev):
    from valor_amd import capeval
    fix = load()
    dm = capeval.DeviceCaptionMetrics(fix["refs"], device=dev, eos=fix["eos"])
    got = dm.score(fix["ids"], fix["seq"].to(dev), per_clip=True)
    host = dm.host.score(fix["ids"], [r[:r.index(fix["eos"])] if fix["eos"] in r else r for r in fix["seq"].tolist()])
    _compare("fixture/host", got, host)
    want = {"ROUGE_L": fix["rouge"].numpy(), "CIDEr": fix["cider"].numpy(), **{f"Bleu_{k + 1}": fix["bleu"][:, k].numpy() for k in range(4)}}
    for k in KEYS:
        np.testing.assert_allclose(got.per_clip[k], want[k], rtol=RTOL, atol=ATOL, err_msg=k)
    np.testing.assert_allclose([got.corpus[k] for k in KEYS], fix["corpus"].numpy(), rtol=RTOL, atol=ATOL)
    assert capeval.rounded(got.corpus) == {k: round(v * 100, 2) for k, v in zip(KEYS, fix["corpus"].tolist())}
    lean = dm.score(fix["ids"], fix["seq"].to(dev))                            # the summary alone: the same bits, nothing per clip
    assert lean.per_clip is None and lean.corpus == got.corpus and lean.totals == got.totals


def test_boundary_lengths_of_hypothesis_and_reference(dev):
    """every hypothesis length around the two 64-bit words against every reference length around them; six symbols, so that the
    common subsequences are long and the carry between the words is exercised"""
    from valor_amd import capeval
    rng = np.random.default_rng(5)
    word = lambda n: rng.integers(1000, 1006, size=n).tolist()
    refs, hyps = {}, []
    for hl in (0, 1, 63, 64, 65, 127, 128):
        for rl in (1, 64, 65, 200):
            refs[f"h{hl}r{rl}"] = [word(rl)] + ([word(rl)] if (hl + rl) % 2 else [])
            hyps.append(word(hl))
    ids = list(refs)
    dm = capeval.DeviceCaptionMetrics(refs, device=dev, eos=EOS)
    got = dm.score(ids, torch.from_numpy(_pad(hyps, 128, rng)).to(dev), per_clip=True)
    want = dm.host.score(ids, hyps)
    _compare("boundary", got, want)
    assert want.per_clip["ROUGE_L"][8:].min() > 0 and (want.per_clip["ROUGE_L"][:4] == 0).all()          # from 63 symbols on something is common
    # the hypothesis itself as the only reference: LCS = the full length at every width
    same = {f"s{n}": [word(n)] for n in (1, 63, 64, 65, 127, 128)}
    ds = capeval.DeviceCaptionMetrics(same, device=dev, eos=EOS)
    res = ds.score(list(same), torch.from_numpy(_pad([r[0] for r in same.values()], 128, rng)).to(dev), per_clip=True)
    np.testing.assert_allclose(res.per_clip["ROUGE_L"], 1.0, rtol=RTOL)
    np.testing.assert_allclose(res.per_clip["Bleu_1"], 1.0, rtol=1e-6)          # the 1e-15 / 1e-9 terms of the law


def test_many_references_beyond_the_lanes_and_the_lds_stage(dev):
    """a clip with 300 references (more than the 256 lanes that walk them, 64 per wave) and ~10 000 n-gram entries (the stage holds
    1536), next to small clips in the same launch; hypotheses with repeated symbols, symbols in no reference and symbols outside the
    vocabulary"""
    from valor_amd import capeval
    rng = np.random.default_rng(6)
    word = lambda n: rng.integers(1000, 1030, size=int(n)).tolist()
    refs = {"big": [word(rng.integers(3, 16)) for _ in range(300)], "mid": [word(rng.integers(3, 16)) for _ in range(70)]}
    refs.update({f"c{i}": [word(rng.integers(3, 16)) for _ in range(int(rng.integers(1, 6)))] for i in range(14)})
    ids = list(refs)
    hyps = [refs["big"][299][:6] + word(4) + refs["big"][257][2:], refs["mid"][69] + refs["mid"][3]]
    hyps += [[1001, 1002] * 5, [5000, 5001, 5000, 5001, 1003], [], word(30)] + [refs[f"c{i}"][0][1:] + word(2) for i in range(6, 14)]
    hyps += [word(7), word(12)]
    assert len(hyps) == len(ids)
    dm = capeval.DeviceCaptionMetrics(refs, device=dev, eos=EOS)
    T = dm.tables_for(ids)
    assert T["ref_key_ptr"][300] > 1536 * 4
    seq = torch.from_numpy(_pad(hyps, 40, rng, lo=1000, hi=1030)).to(dev)
    _compare("many", dm.score(ids, seq, per_clip=True), dm.host.score(ids, hyps))
    # ids outside the vocabulary match nothing but still count as words (and two different ones stay two words)
    odd = [[1000, 70000, 80000, 1001], [1000, 70000, 70000, 1001]]
    small = capeval.DeviceCaptionMetrics({"a": [[1000, 1001, 1002]], "b": [[1000, 7, 7, 1001]]}, device=dev, eos=EOS)
    got = small.score(["a", "b"], torch.tensor([h + [EOS, 1002] for h in odd], device=dev), per_clip=True)
    _compare("outside", got, small.host.score(["a", "b"], odd))


@pytest.fixture(scope="module")
def big_corpus():
    """2990 clips (the MSRVTT test count) of two short references; one hypothesis each. The host results are computed once per size."""
    rng = np.random.default_rng(7)
    word = lambda n: rng.integers(1000, 1200, size=int(n)).tolist()
    refs = {f"v{i}": [word(rng.integers(4, 9)), word(rng.integers(4, 9))] for i in range(2990)}
    hyps = [(r[0][:3] + word(rng.integers(0, 4))) if i % 3 else word(rng.integers(0, 9)) for i, r in enumerate(refs.values())]
    return refs, hyps, _pad(hyps, 12, rng, lo=1000, hi=1200)


@pytest.mark.parametrize("R", [1, 257, 2990])
def test_corpus_reduction_sizes(dev, big_corpus, R):
    from valor_amd import capeval
    refs, hyps, seq = big_corpus
    ids = list(refs)[:R]
    dm = capeval.DeviceCaptionMetrics({i: refs[i] for i in ids}, device=dev, eos=EOS)
    got = dm.score(ids, torch.from_numpy(seq[:R]).to(dev), per_clip=True)
    want = dm.host.score(ids, hyps[:R])
    _compare(f"R={R}", got, want)
    assert got.totals["testlen"] == sum(len(h) for h in hyps[:R])
    if R == 2990:                                                              # the word-list entry: interned, padded and uploaded by score()
        again = dm.score(ids, hyps[:R])
        assert again.corpus == got.corpus and again.totals == got.totals


def test_two_launches_give_the_same_bits_and_a_row_pitch_is_honoured(dev):
    from valor_amd import capeval
    fix = load()
    dm = capeval.DeviceCaptionMetrics(fix["refs"], device=dev, eos=fix["eos"])
    seq = fix["seq"].to(dev)
    a, b = dm.score(fix["ids"], seq, per_clip=True), dm.score(fix["ids"], seq, per_clip=True)
    for k in KEYS + INTS:
        assert np.array_equal(a.per_clip[k], b.per_clip[k], equal_nan=True), k
    assert a.corpus == b.corpus and a.totals == b.totals
    wide = torch.full((seq.shape[0], 160), 1001, dtype=torch.int64, device=dev)
    wide[:, 7:135] = seq
    view = wide[:, 7:135]
    assert view.stride(0) == 160 and not view.is_contiguous()
    c = dm.score(fix["ids"], view, per_clip=True)
    for k in KEYS + INTS:
        assert np.array_equal(a.per_clip[k], c.per_clip[k]), k
    assert a.corpus == c.corpus
    narrow = dm.score(fix["ids"][:60], seq[:60, :30])                          # L = 30: rows without an end mark are cut by the width
    want = dm.host.score(fix["ids"][:60], [r[:r.index(fix["eos"])] if fix["eos"] in r else r for r in fix["seq"][:60, :30].tolist()])
    for k in KEYS:
        np.testing.assert_allclose(narrow.corpus[k], want.corpus[k], rtol=RTOL, atol=ATOL)


def test_nan_rows_and_refused_arguments(dev):
    from valor_amd import capeval, kernels as K, lib, scst
    m = capeval.CaptionMetrics({"a": [[1000, 1001, 1002]], "bare": [], "b": [[1001, 1002], [1002, 1003, 1004]]})
    T = scst.reward_tables(scst.CaptionScorer(m.refs))                         # the reward's builder keeps the clip without references
    flat = [r for refs in m.refs.values() for r in refs]
    T["ref_sym_ptr"] = np.cumsum([0] + [len(r) for r in flat]).astype(np.int32)
    T["ref_syms"] = np.array([t for r in flat for t in r], dtype=np.uint16)
    keep, st = capeval.upload_tables(T, torch.device(dev))
    seq = torch.tensor([[1000, 1001, EOS], [1000, 1001, EOS], [1001, 1002, EOS], [1001, EOS, 0], [1001, EOS, 0]], device=dev)
    clip = torch.tensor([0, 1, 2, 3, -1], dtype=torch.int32, device=dev)       # 'a', the bare clip, 'b', two indices outside the table
    R = 5
    f64 = torch.zeros((6, R), dtype=torch.float64, device=dev)
    counts = torch.zeros((R, 10), dtype=torch.int32, device=dev)
    summary = torch.zeros(16, dtype=torch.int64, device=dev)
    K.caption_metrics(seq, EOS, 2000, clip, st, f64[0], f64[1], f64[2:].view(-1), counts, summary)
    f, c, s = f64.cpu().numpy(), counts.cpu().numpy(), summary.cpu()
    bad = np.array([False, True, False, True, True])
    assert np.isnan(f[:2, bad]).all() and np.isnan(f[2:].reshape(R, 4)[bad]).all() and (c[bad] == -1).all()
    assert np.isfinite(f[:2, ~bad]).all() and (c[~bad, 8] == 2).all()
    assert np.isnan(s[:6].view(torch.float64).numpy()).all()                   # a NaN row makes the summary NaN
    assert s[6:].tolist() == c[~bad].sum(axis=0).tolist()                      # the totals cover the other rows
    want = capeval.metrics_from_tables(T, clip.cpu().numpy(), seq.cpu().numpy(), EOS, 2000)
    np.testing.assert_allclose(f[0], want.per_clip["CIDEr"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(f[1], want.per_clip["ROUGE_L"], rtol=RTOL, atol=ATOL)
    # R == 0: nothing launched, the summary zeroed
    summary.fill_(-1)
    K.caption_metrics(seq[:0], EOS, 2000, clip[:0], st, f64[0, :0], f64[1, :0], f64[2:, :0].reshape(-1), counts[:0], summary)
    assert summary.cpu().tolist() == [0] * 16
    # VALOR_ERR_ARG: rows wider than 128, a vocabulary the keys cannot carry, an end mark outside it
    wide = torch.zeros((R, 129), dtype=torch.int64, device=dev)
    for bad_call in (lambda: K.caption_metrics(wide, EOS, 2000, clip, st, f64[0], f64[1], f64[2:].view(-1), counts, summary),
                     lambda: K.caption_metrics(seq, EOS, 65535, clip, st, f64[0], f64[1], f64[2:].view(-1), counts, summary),
                     lambda: K.caption_metrics(seq, 2000, 2000, clip, st, f64[0], f64[1], f64[2:].view(-1), counts, summary)):
        with pytest.raises(lib.ValorHipError):
            bad_call()
    dm = capeval.DeviceCaptionMetrics({"a": [[1000, 1001]]}, device=dev, eos=EOS)
    with pytest.raises(ValueError):
        dm.score(["a"], wide[:1])
    with pytest.raises(ValueError):
        dm.score(["a"], seq[:2])
    with pytest.raises(lib.ValorHipError):
        dm.score(["a"], seq[:1].cpu())                                         # no CPU fallback
    assert keep


def one_scorer_case(L):
    """the corpus and the rows of test_the_two_entry_points_are_one_scorer -> (references, int64 [31, L] rows, int32 [31] clip indices).
    Five clips with 3 references of 3..12 tokens and one with 40 references of 14; per clip an empty row, one token, an exact reference,
    a row with an id outside the vocabulary (2000) and one repeated token over the full width without an end mark; last, a row of clip -1."""
    rng = np.random.default_rng(11)
    word = lambda n: rng.integers(1000, 1200, size=int(n)).tolist()
    refs = {f"c{i}": [word(rng.integers(3, 13)) for _ in range(3)] for i in range(5)}
    refs["big"] = [word(14) for _ in range(40)]
    hyps, clip = [], []
    for c, r in enumerate(refs.values()):
        hyps += [[], r[0][:1], r[0], r[1][:2] + [5000] + r[1][2:], r[2][:1] * L]
        clip += [c] * 5
    hyps.append(r[0])
    clip.append(-1)
    return refs, _pad(hyps, L, rng, lo=1000, hi=1200), np.array(clip, dtype=np.int32)


@pytest.mark.parametrize("L", [30, 128])
def test_the_two_entry_points_are_one_scorer(dev, L):
    """valor_caption_metrics and valor_caption_reward run one n-gram core (csrc/ngram.h): on the same rows and the same references their
    CIDEr values, and Bleu_4 / BLEU-4, are the same bits -- through the LDS stage (the small clips) and past it (the clip of ~2000 keys)"""
    from valor_amd import capeval, kernels as K, scst
    refs, rows, clip = one_scorer_case(L)
    T = capeval.capeval_tables(capeval.CaptionMetrics(refs), list(refs))
    big = list(refs).index("big")
    assert T["ref_key_ptr"][T["clip_ref_ptr"][big + 1]] - T["ref_key_ptr"][T["clip_ref_ptr"][big]] > 1536
    keep, st = capeval.upload_tables(T, torch.device(dev))
    seq, R = torch.from_numpy(rows).to(dev), len(clip)
    assert (seq[4::5, :] != EOS).all() and seq.shape == (31, L)
    f64 = torch.zeros((6, R), dtype=torch.float64, device=dev)
    counts = torch.zeros((R, 10), dtype=torch.int32, device=dev)
    summary = torch.zeros(16, dtype=torch.int64, device=dev)
    K.caption_metrics(seq, EOS, 2000, torch.from_numpy(clip).to(dev), st, f64[0], f64[1], f64[2:].view(-1), counts, summary)
    _, cider, bleu4 = scst.DeviceCaptionScorer(refs, device=dev, vocab=2000).score(clip, seq, EOS, parts=True)
    bits = lambda t: t.contiguous().view(torch.int64).cpu()
    print(f"[capeval one scorer L={L}] CIDEr {f64[0, :5].tolist()} .. BLEU-4 {bleu4[:5].tolist()}")
    assert torch.equal(bits(f64[0]), bits(cider))
    assert torch.equal(bits(f64[2:].view(R, 4)[:, 3]), bits(bleu4))
    assert torch.isnan(f64[0, -1]) and torch.isnan(cider[-1]) and torch.isnan(f64[2:].view(R, 4)[-1]).all() and torch.isnan(bleu4[-1])
    assert torch.isfinite(f64[0, :-1]).all() and (f64[0, 2::5] > 0).all() and (counts[:-1:5, 8] == 0).all() and (counts[4::5, 8] == L).all()
    assert keep


# ------------------------------------------------------------------ end to end: validate_cap / validate_qa on the small synthetic model
OPTS = {"dropout": 0.0, "drop_path_rate": 0.0, "beam_size": 1, "max_generation_len": 8}


def _shards(questions=False):
    from valor_amd import synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    bs = []
    for i, n in enumerate((3, 2, 4)):
        b = synth.make_batch(spec, batch=n, frames=2, audio_slices=1, txt_len=10, seed=20 + i, questions=questions)
        b["ids"] = [f"v{10 * i + j}" for j in range(n)]
        if questions:
            b["question_ids"] = [f"q{10 * i + j}" for j in range(n)]
        bs.append(b)
    return spec, sd, [[bs[0], bs[2]], [bs[1]]]                                 # two unequal shards: 7 clips and 2


def _model(spec, sd, dev):
    from valor_amd.model.valor import VALOR
    m = VALOR(dict(OPTS), spec=spec, dtype=torch.float32, device=dev)
    m.load_state_dict(sd, strict=True)
    return m


def _references(spec, batches):
    """seeded references over the synthetic vocabulary's words (no model needed: the ranks of the gloo test build the same ones)"""
    rng = np.random.default_rng(9)
    word = lambda n: [f"[unused{int(t)}]" for t in rng.integers(104, spec.vocab, size=int(n))]
    return {i: [" ".join(word(rng.integers(3, 9))) for _ in range(int(rng.integers(1, 4)))] for b in batches for i in b["ids"]}


def _overlapping_references(model, spec, batches):
    """the seeded references plus, per clip, two that share words with what the model generates for the tv group, so that the metrics
    are not all zero -> (references, {clip id: the generated tv caption})"""
    sents = {}
    for b in batches:
        ev = model(b, task="cap%tv", compute_loss=False)
        sents.update(zip(b["ids"], model.decode_sequence(ev["generated_sequences_t_v"])))
    rng = np.random.default_rng(3)
    refs = _references(spec, batches)
    for i, s in sents.items():
        w = s.split()
        refs[i].append(" ".join(w[:max(1, len(w) - 2)] + ["[unused150]"]))
        refs[i].append(" ".join(x for x in w if rng.random() < 0.7) or "[unused151]")
    return refs, sents


def test_validate_cap_device_equals_host_and_writes_the_results(dev, tmp_path):
    from valor_amd import capeval
    from valor_amd.evaluate import validate_cap
    spec, sd, shards = _shards()
    batches = [b for s in shards for b in s]
    model = _model(spec, sd, dev)
    model.train()
    refs, sents = _overlapping_references(model, spec, batches)
    task = "cap%tv%tva%ta"
    device_log = validate_cap(model, batches, task, refs, scorer="device", output_dir=str(tmp_path), global_step=11, dset_name="syn")
    host_log = validate_cap(model, batches, task, refs, scorer="host")
    print("[capeval e2e]", device_log)
    assert device_log == host_log and list(device_log) == ["tva", "tv", "ta"] and all(set(v) == set(KEYS) for v in device_log.values())
    assert device_log["tv"]["Bleu_1"] > 0 and device_log["tv"]["ROUGE_L"] > 0 and device_log["tv"]["CIDEr"] > 0
    for g in ("tva", "tv", "ta"):
        out = json.load(open(tmp_path / "results_test_syn" / f"step_11_{g}.json"))
        assert [r["video_id"] for r in out] == [i for b in batches for i in b["ids"]] and all(isinstance(r["caption"], str) and set(r) == {"video_id", "caption"} for r in out)
    out = json.load(open(tmp_path / "results_test_syn" / "step_11_tv.json"))
    assert {r["video_id"]: r["caption"] for r in out} == sents
    # the file's captions scored by the host scorer give the log
    host = capeval.CaptionMetrics(refs, tokenize=capeval.simple_tokenize)
    assert capeval.rounded(host.score([r["video_id"] for r in out], [r["caption"] for r in out]).corpus) == device_log["tv"]
    # a scorer kept across rounds builds its tables once
    from valor_amd.evaluate import caption_metrics_for
    kept = caption_metrics_for(refs, device=dev)
    assert validate_cap(model, batches, "cap%tv", kept) == {"tv": device_log["tv"]}
    tables = kept._dev
    assert validate_cap(model, batches, "cap%tv", kept) == {"tv": device_log["tv"]} and kept._dev is tables


def _qa_truth(model, batches):
    """ground-truth answer strings: the model's own tv answer for every other question, the training rows' answers for the rest"""
    out = []
    for b in batches:
        pred = model.decode_sequence(model(b, task="qa%tv", compute_loss=False)["generated_answers_t_v"])
        given = model.decode_sequence(b["txt_tokens"]["bert_tokens"][:, 1:])
        out.append([p if (j % 2 == 0) else g for j, (p, g) in enumerate(zip(pred, given))])
    return out


def test_validate_qa_accuracy_equals_a_restatement(dev, tmp_path):
    from valor_amd.evaluate import validate_qa
    spec, sd, shards = _shards(questions=True)
    batches = [b for s in shards for b in s]
    model = _model(spec, sd, dev)
    batches = [dict(b, answers=a) for b, a in zip(batches, _qa_truth(model, batches))]
    log = validate_qa(model, batches, "qa%tv%tva", output_dir=str(tmp_path), global_step=2, dset_name="syn")
    gt = [a for b in batches for a in b["answers"]]
    for g, key in (("tv", "generated_answers_t_v"), ("tva", "generated_answers_t_va")):
        pred = [s for b in batches for s in model.decode_sequence(model(b, task="qa%tv%tva", compute_loss=False)[key])]
        assert log[g] == {"accuracy": round(sum(p == t for p, t in zip(pred, gt)) / len(gt) * 100, 2)}
    print("[capeval qa]", log)
    assert 50.0 <= log["tv"]["accuracy"] <= 100.0 and set(log) == {"tv", "tva"}
    folder = tmp_path / "predict_answers"
    assert json.load(open(folder / "step2_gt.json")) == gt
    sub = json.load(open(folder / "step2_tv_pred_submited_syn.json"))
    assert [s["question_id"] for s in sub] == [q for b in batches for q in b["question_ids"]]
    assert [s["answer"] for s in sub] == json.load(open(folder / "step2_tv_pred.json"))
    # the training schema (token rows as ground truth) is decoded like the predictions
    plain = validate_qa(model, [{k: v for k, v in b.items() if k != "answers"} for b in batches], "qa%tv")
    assert 0.0 <= plain["tv"]["accuracy"] <= 100.0


def _eval_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        from valor_amd.evaluate import validate_cap, validate_qa
        torch.cuda.set_device(0)
        given = torch.load(os.path.join(outdir, "given.pt"), weights_only=False)          # the parent's references and answers
        spec, sd, shards = _shards()
        model = _model(spec, sd, "cuda:0")
        cap = validate_cap(model, shards[rank], "cap%tv%tva", given["refs"], output_dir=outdir, global_step=1, dset_name="two")
        spec, sd, qshards = _shards(questions=True)
        qa = validate_qa(model, [dict(b, answers=given["answers"][b["ids"][0]]) for b in qshards[rank]], "qa%tv%tva",
                         output_dir=outdir, global_step=1, dset_name="two")
        torch.save((cap, qa), os.path.join(outdir, f"eval{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_validate_cap_and_qa_gather_the_ranks_shards(dev, tmp_path):
    """two ranks (gloo, one GPU) with unequal shards return, each, the log one process returns for the shards in rank order. The
    references and answers overlap what the model generates, so that log is not trivial, and it differs from the log of either shard
    alone: a rank that scored only its own shard, or gathered in another order, would not return it."""
    import socket
    from valor_amd.evaluate import validate_cap, validate_qa
    spec, sd, shards = _shards()
    model = _model(spec, sd, dev)
    batches = [b for s in shards for b in s]
    refs, _ = _overlapping_references(model, spec, batches)
    qshards = _shards(questions=True)[2]
    qbatches = [b for s in qshards for b in s]
    answers = {b["ids"][0]: a for b, a in zip(qbatches, _qa_truth(model, qbatches))}          # a batch is named by its first clip
    with_answers = lambda bs: [dict(b, answers=answers[b["ids"][0]]) for b in bs]
    torch.save(dict(refs=refs, answers=answers), tmp_path / "given.pt")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_eval_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    logs = [torch.load(tmp_path / f"eval{r}.pt", weights_only=False) for r in range(2)]
    one_cap = validate_cap(model, batches, "cap%tv%tva", refs)
    one_qa = validate_qa(model, with_answers(qbatches), "qa%tv%tva")
    print("[capeval two ranks]", one_cap, one_qa)
    assert set(one_cap) == {"tv", "tva"} and set(one_cap["tv"]) == set(KEYS)
    for g in ("tv", "tva"):
        assert one_cap[g]["Bleu_1"] > 0 and one_cap[g]["ROUGE_L"] > 0 and one_cap[g]["CIDEr"] > 0, g
    assert 0.0 < one_qa["tv"]["accuracy"] < 100.0
    for shard, qshard in zip(shards, qshards):                                 # what a rank without the gather would return
        alone_cap, alone_qa = validate_cap(model, shard, "cap%tv%tva", refs), validate_qa(model, with_answers(qshard), "qa%tv%tva")
        print("[capeval one shard]", alone_cap, alone_qa)
        assert alone_cap["tv"] != one_cap["tv"] and alone_cap["tva"] != one_cap["tva"] and alone_qa["tv"] != one_qa["tv"]
    assert logs[0] == (one_cap, one_qa) and logs[1] == (one_cap, one_qa), (logs, one_cap, one_qa)
    out = json.load(open(tmp_path / "results_test_two" / "step_1_tv.json"))
    assert [r["video_id"] for r in out] == [i for b in batches for i in b["ids"]]
    # the gathered answers, ground truth and submission list are in rank order: shard 0's batches, then shard 1's
    folder = tmp_path / "predict_answers"
    assert json.load(open(folder / "step1_gt.json")) == [a for b in with_answers(qbatches) for a in b["answers"]]
    assert [x["question_id"] for x in json.load(open(folder / "step1_tv_pred_submited_two.json"))] == [q for b in qbatches for q in b["question_ids"]]
