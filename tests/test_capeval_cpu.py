"""CPU: the caption evaluation metrics (valor_amd.capeval) -- the host scorer CaptionMetrics against the fixture of the UNMODIFIED
reference's Bleu / Rouge / Cider (tests/golden/cap_metrics.pt, tools/make_capeval_goldens.py), the numpy walker of the device tables
against the host scorer, simple_tokenize, VALOR.decode_sequence, the errors, the argument checks of valor_caption_metrics without a GPU,
and validate_qa / validate routing with a stub model.

Tolerance of every fp64 comparison: rtol 1e-9, atol 1e-12, the one derived at the top of tests/test_reward_cpu.py: the sums have
non-negative terms, at most a few thousand of them, so a reordered sum or mean moves by ~1e-13 relative; exp / sqrt / pow differ between
implementations by a few ulp. Integers are compared exactly. No row is excluded."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_capeval_goldens import EDGE_LENGTHS, KEYS, boundary_margin, load  # noqa: E402  (one definition for fixture and tests)
from valor_amd import capeval, scst  # noqa: E402

RTOL, ATOL = 1e-9, 1e-12
close = lambda a, b: np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


@pytest.fixture(scope="module")
def fix():
    f = load()                                                                 # numbers and tensors only: torch.load(weights_only=True)
    f["hyps"] = scst.hypotheses(f["seq"], f["eos"])
    f["host"] = capeval.CaptionMetrics(f["refs"])
    f["want"] = f["host"].score(f["ids"], f["hyps"])
    return f


def test_fixture_covers_the_cases(fix):
    assert sorted(fix["ids"]) == sorted(fix["refs"]) and len(set(fix["ids"])) == len(fix["ids"]) == 68          # every clip exactly once
    assert len(fix["refs"]["many"]) > 64 and max(len(r) for r in fix["refs"]["long"]) > 128
    lens = [len(h) for h in fix["hyps"]]
    assert set(EDGE_LENGTHS) | {0} <= set(lens) and fix["seq"].shape == (68, 128)
    assert boundary_margin(fix["corpus"].tolist()) > 1e-6                      # the rounded dict may be compared for equality
    T = capeval.capeval_tables(fix["host"], fix["ids"])
    c = fix["ids"].index("many")
    assert T["ref_key_ptr"][T["clip_ref_ptr"][c + 1]] - T["ref_key_ptr"][T["clip_ref_ptr"][c]] > 1536          # beyond the kernel's LDS stage


def test_host_scorer_equals_the_reference_fixture(fix):
    got = fix["want"]
    for k in range(4):
        close(got.per_clip[f"Bleu_{k + 1}"], fix["bleu"][:, k].numpy())
    close(got.per_clip["ROUGE_L"], fix["rouge"].numpy())
    close(got.per_clip["CIDEr"], fix["cider"].numpy())
    close([got.corpus[k] for k in KEYS], fix["corpus"].numpy())
    assert capeval.rounded(got.corpus) == {k: round(v * 100, 2) for k, v in zip(KEYS, fix["corpus"].tolist())}
    assert tuple(got.corpus) == KEYS and "METEOR" not in got.corpus
    empty = fix["hyps"].index([])
    assert got.per_clip["ROUGE_L"][empty] == 0 and got.per_clip["CIDEr"][empty] == 0 and got.per_clip["testlen"][empty] == 0
    assert got.totals["testlen"] == sum(len(h) for h in fix["hyps"]) and got.totals["guess"][0] == got.totals["testlen"]


def test_table_walker_equals_the_host_scorer(fix):
    dev = capeval.DeviceCaptionMetrics(fix["host"], eos=fix["eos"])
    T = dev.tables_for(fix["ids"])
    assert T["clips"] == fix["ids"] and T["ref_syms"].dtype == np.uint16 and T["ref_sym_ptr"][-1] == len(T["ref_syms"])
    assert T["ref_len"] == np.log(68.0)                                        # df and ref_len over the evaluated clips
    got = capeval.metrics_from_tables(T, np.arange(68, dtype=np.int32), fix["seq"].numpy(), fix["eos"])
    for k in KEYS:
        close(got.per_clip[k], fix["want"].per_clip[k])
        close(got.corpus[k], fix["want"].corpus[k])
    for k in ("correct", "guess", "testlen", "reflen"):
        assert (got.per_clip[k] == fix["want"].per_clip[k]).all(), k
    assert got.totals == fix["want"].totals
    # a subset of the clips is another corpus: the document frequency follows the evaluated clips
    sub = fix["ids"][5:25]
    a = capeval.metrics_from_tables(capeval.capeval_tables(fix["host"], sub), np.arange(20), fix["seq"].numpy()[5:25], fix["eos"])
    b = fix["host"].score(sub, fix["hyps"][5:25])
    close(a.per_clip["CIDEr"], b.per_clip["CIDEr"])
    assert not np.allclose(b.per_clip["CIDEr"], fix["want"].per_clip["CIDEr"][5:25])
    # a row without a clip: NaN values, -1 integers, NaN corpus
    bad = capeval.metrics_from_tables(T, np.array([0, 99, -1]), fix["seq"].numpy()[:3], fix["eos"])
    assert np.isnan(bad.per_clip["CIDEr"][1:]).all() and (bad.per_clip["testlen"][1:] == -1).all() and all(np.isnan(v) for v in bad.corpus.values())
    assert np.isfinite(bad.per_clip["CIDEr"][0])


def test_bit_parallel_lcs_equals_the_table_recurrence():
    rng = np.random.default_rng(0)
    for _ in range(300):
        a = rng.integers(0, 6, size=int(rng.integers(0, 140))).tolist()
        b = rng.integers(0, 6, size=int(rng.integers(0, 220))).tolist()
        assert capeval._bit_lcs(a, b) == capeval.lcs_length(a, b) == capeval.lcs_length(b, a)
    assert capeval.lcs_length("abcbdab", "bdcaba") == 4 and capeval._bit_lcs([], [1, 2]) == 0


def test_words_are_interned_and_strings_equal_integers(fix):
    """the same corpus as word strings scores the same: symbols are only names"""
    word = lambda seq: [f"w{t}" for t in seq]
    refs = {i: [word(r) for r in rs] for i, rs in fix["refs"].items()}
    m = capeval.CaptionMetrics(refs)
    assert m.interned and m.n_symbols == len({t for rs in fix["refs"].values() for r in rs for t in r}) + 1
    got = m.score(fix["ids"], [word(h) for h in fix["hyps"]])
    for k in KEYS:
        close(got.per_clip[k], fix["want"].per_clip[k])
    assert got.totals == fix["want"].totals
    sym, vocab = m.encode([word(fix["hyps"][2])])                              # kind 2: words in no reference get numbers of their own
    assert min(sym[0]) >= m.n_symbols and vocab == m.n_symbols + len(set(sym[0])) and capeval.END not in sym[0]
    assert m.encode([["w1000"]])[1] == m.n_symbols                             # the overlay lives for one call
    dm, vocab = capeval.DeviceCaptionMetrics(m).id_matrix([word(h) for h in fix["hyps"][:4]])
    assert dm.dtype == np.int64 and dm.shape[0] == 4 and (dm[0] == capeval.END).all() and scst.hypotheses(dm, capeval.END)[1] == m.encode([word(fix["hyps"][1])])[0][0]
    with_tok = capeval.CaptionMetrics({"a": ["A man, a plan."]}, tokenize=capeval.simple_tokenize)
    assert with_tok.score(["a"], ["a man a plan"]).corpus["Bleu_4"] == pytest.approx(1.0, abs=1e-6)
    with pytest.raises(TypeError):
        capeval.CaptionMetrics({"a": ["no tokenizer given"]})
    with pytest.raises(TypeError):
        capeval.CaptionMetrics({"a": [["word", 3]]})


def test_simple_tokenize():
    t = capeval.simple_tokenize
    assert t("A man is  playing\tthe Guitar.") == ["a", "man", "is", "playing", "the", "guitar"]
    assert t("hello , world !") == ["hello", "world"] and t("...") == [] and t("") == []
    assert t("the man's dog (brown) isn't here") == ["the", "man", "s", "dog", "brown", "isn", "t", "here"]          # not PTB: see the docstring
    assert t("well-known 3d_model") == ["well", "known", "3d", "model"]


def test_duplicate_unknown_and_oversized_errors(fix):
    m = fix["host"]
    with pytest.raises(ValueError, match="clip7"):
        m.score(["clip7", "clip8", "clip7"], [[1000]] * 3)
    with pytest.raises(KeyError):
        m.score(["clip7", "nowhere"], [[1000]] * 2)
    with pytest.raises(ValueError):
        m.score(["clip7"], [[1000]] * 2)
    bare = capeval.CaptionMetrics(dict(fix["refs"], bare=[]))
    with pytest.raises(ValueError, match="bare"):
        bare.score(["bare"], [[1000]])
    dev = capeval.DeviceCaptionMetrics(m, eos=fix["eos"])
    for call in (lambda: dev.tables_for(["clip7", "clip7"]), lambda: capeval.capeval_tables(bare, ["clip1", "bare"])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(KeyError):
        dev.tables_for(["nowhere"])
    with pytest.raises(ValueError, match="eos"):
        capeval.DeviceCaptionMetrics(m)                                        # integer words: the caller names the end mark
    # a vocabulary the 16-bit keys cannot carry: the references', or the references' plus the new hypothesis words
    big = capeval.CaptionMetrics({"a": [[1, scst.MAX_TOKEN + 1]]})
    with pytest.raises(ValueError, match="host scorer"):
        capeval.capeval_tables(big, ["a"])
    words = capeval.CaptionMetrics({"a": [[f"w{i}" for i in range(scst.MAX_VOCAB - 10)]]})
    wd = capeval.DeviceCaptionMetrics(words)
    assert wd.id_matrix([["w1", "w2"]])[1] == scst.MAX_VOCAB - 9
    with pytest.raises(ValueError, match="host scorer"):
        wd.id_matrix([[f"new{i}" for i in range(20)]])
    with pytest.raises(ValueError, match="host scorer"):
        capeval.DeviceCaptionMetrics(m, eos=fix["eos"]).id_matrix([[1000] * 129])
    assert words.score(["a"], [[f"new{i}" for i in range(20)]]).corpus["CIDEr"] == 0          # the host scorer takes it
    empty = m.score([], [])
    assert empty.corpus == dict.fromkeys(KEYS, 0.0) and empty.totals["testlen"] == 0


def test_decode_sequence():
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    toks = synth.synthetic_vocab(400)
    toks[300:304] = ["play", "##ing", "guitar", "##s"]
    m = VALOR.__new__(VALOR)                                                   # decode_sequence reads three attributes, no parameters
    m.vocab_tokens, m.eos_token, m.tokenizer_type = toks, 102, "bert"
    seq = torch.tensor([[300, 301, 302, 303, 102, 300], [302, 102, 102, 102, 102, 102], [102, 300, 300, 300, 300, 300], [300, 302, 300, 302, 300, 302]])
    assert m.decode_sequence(seq) == ["playing guitars", "guitar", "", "play guitar play guitar play guitar"]
    m.tokenizer_type = "clip"
    with pytest.raises(NotImplementedError):
        m.decode_sequence(seq)


def test_caption_metrics_validates_arguments_without_gpu():
    from valor_amd import lib
    so = lib.load()
    assert "valor_caption_metrics" in lib.SIGNATURES
    i64 = (ctypes.c_int64 * 1024)()
    i32 = (ctypes.c_int32 * 64)()
    f64 = (ctypes.c_double * 64)()
    buf = ctypes.addressof(i64)
    tab = lib.CapevalTables()
    for k in lib.CapevalTables.POINTERS:
        setattr(tab, k, buf)
    tab.ref_len, tab.n_global, tab.n_clips = 1.0, 4, 2
    assert ctypes.sizeof(tab) == 14 * 8 + 8 + 2 * 4 and ctypes.sizeof(lib.CapevalSummary) == 16 * 8
    summ = lib.CapevalSummary()

    def call(R=4, L=30, ld=30, eos=0, vocab=30522, seq=i64, clip=i32, tables=tab, cider=f64, rouge=f64, bleu=f64, counts=i32, summary=summ):
        t = None if tables is None else ctypes.addressof(tables)
        s = None if summary is None else ctypes.addressof(summary)
        return so.valor_caption_metrics(None, seq, ld, R, L, eos, vocab, clip, t, cider, rouge, bleu, counts, s)
    assert call(R=-1) == -1 and call(L=0) == -1 and call(L=129, ld=129) == -1 and call(ld=29) == -1
    assert call(vocab=65535) == -1 and call(vocab=0) == -1 and call(eos=30522) == -1 and call(eos=-1) == -1
    assert call(seq=None) == -1 and call(clip=None) == -1 and call(tables=None) == -1
    assert call(cider=None) == -1 and call(rouge=None) == -1 and call(bleu=None) == -1 and call(counts=None) == -1 and call(summary=None) == -1
    for k in lib.CapevalTables.POINTERS:
        broken = lib.CapevalTables.from_buffer_copy(tab)
        setattr(broken, k, None)
        assert call(tables=broken) == -1, k
    assert call(R=0, summary=None) == 0 and call(R=0, seq=None, cider=None, summary=None) == 0          # no rows, no summary: no-op
    assert call(R=0, L=128, ld=128, vocab=65534, eos=65533, summary=None) == 0                           # the largest geometry is inside the domain
    assert call(R=0, L=129, ld=129, summary=None) == -1


def test_capeval_structs_are_one_layout_in_header_binding_and_kernel():
    from valor_amd import lib
    hdr = open(os.path.join(ROOT, "include", "valor_hip.h")).read()
    assert "int valor_caption_metrics(" in hdr and "R == 0" in hdr
    body = re.search(r"typedef struct valor_capeval_tables \{(.*?)\} valor_capeval_tables;", hdr, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(const\s+\w+\s*\*|\w+)\s*(\w+(?:\s*,\s*\w+)*)", decl)
            assert m, decl
            fields += [(n.strip(), "ptr" if "*" in m.group(1) else m.group(1)) for n in m.group(2).split(",")]
    ctypes_of = {"ptr": ctypes.c_void_p, "double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(lib.CapevalTables._fields_)
    assert tuple(n for n, t in fields if t == "ptr") == lib.CapevalTables.POINTERS
    off = 0
    for n, t in fields:
        assert getattr(lib.CapevalTables, n).offset == off, n
        off += ctypes.sizeof(ctypes_of[t])
    assert off == ctypes.sizeof(lib.CapevalTables)
    assert re.search(r"typedef struct valor_capeval_summary \{\s*double value\[6\];\s*int64_t total\[10\];\s*\} valor_capeval_summary;", hdr)
    assert lib.CapevalSummary.value.offset == 0 and lib.CapevalSummary.total.offset == 48
    src = open(os.path.join(ROOT, "valor_amd", "csrc", "capeval.hip")).read()
    assert '#include "../../include/valor_hip.h"' in src and not re.search(r"\bstruct\s+\w+\s*\{", src)
    T = capeval.capeval_tables(capeval.CaptionMetrics({"a": [[1, 2, 3]], "b": [[2, 3]]}), ["b", "a"])
    assert set(lib.CapevalTables.POINTERS) <= set(T) and T["clips"] == ["b", "a"] and T["ref_syms"].tolist() == [2, 3, 1, 2, 3]


def test_reward_and_metrics_kernels_share_one_ngram_core():
    """csrc/ngram.h is the one definition of the n-gram passes: both kernels include it, no helper is defined in two of the three files,
    and for the same references the two table builders give the same twelve shared arrays"""
    import itertools
    from valor_amd import lib
    src = {f: open(os.path.join(ROOT, "valor_amd", "csrc", f)).read() for f in ("reward.hip", "capeval.hip", "ngram.h")}
    assert '#include "ngram.h"' in src["reward.hip"] and '#include "ngram.h"' in src["capeval.hip"]
    names = {f: set(re.findall(r"DEVINL\s+[\w:<> ]+\s+(\w+)\(", text)) for f, text in src.items()}
    assert {"ng_find", "ng_wave_sum", "ng_bleu", "ng_load_row", "ng_score_slots", "ng_norms", "ng_cider", "ng_cider_total", "ng_correct"} <= names["ngram.h"]
    for a, b in itertools.combinations(names, 2):
        assert not names[a] & names[b], (a, b, names[a] & names[b])
    assert not re.search(r"#define\s+(RW|CE)_(THREADS|WAVES|MAXL|SLOTS|STAGE|UNKNOWN)\b", src["reward.hip"] + src["capeval.hip"])
    rng = np.random.default_rng(4)
    refs = {f"c{i}": [rng.integers(0, 50, size=int(rng.integers(1, 12))).tolist() for _ in range(int(rng.integers(1, 5)))] for i in range(9)}
    ce, rw = capeval.capeval_tables(capeval.CaptionMetrics(refs), list(refs)), scst.reward_tables(scst.CaptionScorer(refs))
    assert len(lib.RewardTables.POINTERS) == 12 and ce["clips"] == rw["clips"] and ce["ref_len"] == rw["ref_len"]
    for k in lib.RewardTables.POINTERS:
        assert ce[k].dtype == rw[k].dtype and np.array_equal(ce[k], rw[k]) and ce[k].size, k


class _StubModel:
    """what validate / validate_qa / validate_cap touch of a model: eval / train, the compute_loss=False call, decode_sequence, opts"""

    def __init__(self, opts=None):
        self.opts, self.device, self.training, self.calls = opts or {}, "cpu", True, []
        self.words = ["[PAD]", "yes", "no", "a", "dog", "run", "##ning", "[SEP]"]

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def decode_sequence(self, seq):
        out = []
        for row in seq.tolist():
            row = row[:row.index(7)] if 7 in row else row
            out.append(" ".join(self.words[t] for t in row).replace(" ##", ""))
        return out

    def __call__(self, batch, task, compute_loss=True):
        assert compute_loss is False and not self.training
        self.calls.append(task)
        if task.startswith("qa"):
            return {"generated_answers_t_v": batch["pred_tv"], "generated_answers_t_va": batch["pred_tva"]}
        return {"generated_sequences_t_v": batch["pred_tv"], "generated_sequences_t_va": batch["pred_tva"]}


def _qa_loader():
    t = torch.tensor
    return [dict(ids=[0, 1], txt_tokens=["yes", "a dog"], question_ids=["q0", "q1"], pred_tv=t([[1, 7, 2], [3, 4, 7]]),
                 pred_tva=t([[2, 7, 7], [3, 4, 7]])),
            dict(ids=[2], txt_tokens={"bert_tokens": t([[0, 5, 6, 7]])}, question_ids=None, pred_tv=t([[5, 6, 7]]), pred_tva=t([[5, 7, 7]]))]


def test_validate_qa_with_a_stub_model(tmp_path):
    from valor_amd.evaluate import validate_qa
    m = _StubModel()
    log = validate_qa(m, _qa_loader(), "qa%tv%tva", output_dir=str(tmp_path), global_step=7, dset_name="msrvtt")
    assert log == {"tv": {"accuracy": 100.0}, "tva": {"accuracy": 33.33}}      # ground truth: yes / a dog / running
    folder = tmp_path / "predict_answers"
    assert json.load(open(folder / "step7_gt.json")) == ["yes", "a dog", "running"]
    assert json.load(open(folder / "step7_tv_pred.json")) == ["yes", "a dog", "running"]
    assert json.load(open(folder / "step7_tv_pred_submited_msrvtt.json")) == [{"question_id": "q0", "answer": "yes"}, {"question_id": "q1", "answer": "a dog"}]
    assert validate_qa(m, _qa_loader(), "qa%tva", decode=lambda seq: ["x"] * len(seq)) == {"tva": {"accuracy": 33.33}}          # the caller's decoder also reads the token-row ground truth of the last batch


def test_validate_routes_the_task_families(tmp_path, monkeypatch):
    from valor_amd import evaluate as E
    seen = []
    monkeypatch.setattr(E, "validate_pt", lambda model, loader, task: seen.append(("pt", task)) or {"pt": 1})
    monkeypatch.setattr(E, "validate_ret", lambda model, loader, task: seen.append(("ret", task)) or {"ret": 1})
    m = _StubModel()
    refs = {0: [["a", "dog"], ["a", "dog", "run"]], 1: ["A dog!"], 2: [["a", "dog", "running"]]}
    cap = [dict(ids=[0, 1], pred_tv=torch.tensor([[3, 4, 7], [3, 4, 5]]), pred_tva=torch.tensor([[3, 4, 5], [7, 7, 7]])),
           dict(ids=[2], pred_tv=torch.tensor([[3, 4, 5, 6, 7]]), pred_tva=torch.tensor([[4, 3, 7, 7, 7]]))]
    loaders = {"pt_contra%tv--a": [], "ret%tv--b": [], "cap%tv%tva--c": cap, "qa%tv--d": _qa_loader()}
    log = E.validate(m, loaders, annotations={"c": refs}, scorer="host", output_dir=str(tmp_path), global_step=3)
    assert m.training and seen == [("pt", "pt_contra%tv"), ("ret", "ret%tv")]
    assert log["pt_contra%tv--a"] == {"pt": 1} and log["ret%tv--b"] == {"ret": 1} and log["qa%tv--d"] == {"tv": {"accuracy": 100.0}}
    c = log["cap%tv%tva--c"]
    assert list(c) == ["tva", "tv"] and set(c["tv"]) == set(KEYS)
    host = capeval.CaptionMetrics(refs, tokenize=capeval.simple_tokenize)
    assert c["tv"] == capeval.rounded(host.score([0, 1, 2], ["a dog", "a dog run", "a dog running"]).corpus)
    assert c["tva"] == capeval.rounded(host.score([0, 1, 2], ["a dog run", "", "dog a"]).corpus)
    assert c["tv"]["Bleu_1"] == 87.5 and c["tv"]["ROUGE_L"] > c["tva"]["ROUGE_L"]          # by hand: 2/2 + 2/3 + 3/3 unigrams = 7/8, no brevity penalty (8 > 7)
    out = json.load(open(tmp_path / "results_test_c" / "step_3_tv.json"))
    assert out == [{"video_id": 0, "caption": "a dog"}, {"video_id": 1, "caption": "a dog run"}, {"video_id": 2, "caption": "a dog running"}]
    # the reference's annotation file, and the submission switches: a submission file and no metrics for that group
    ann = tmp_path / "ann.json"
    ann.write_text(json.dumps({"annotations": [{"video_id": f"v_{i}", "caption": " ".join(r) if isinstance(r, list) else r} for i, rs in refs.items() for r in rs]}))
    named = [dict(b, ids=[f"v_{i}" for i in b["ids"]]) for b in cap]
    assert E.validate_cap(m, named, "cap%tv", str(ann), scorer="host") == {"tv": c["tv"]}
    sub = E.validate_cap(_StubModel({"coco_submit": True, "vatex_submit": True}), named, "cap%tv%tva", str(ann), scorer="host", output_dir=str(tmp_path), dset_name="s")
    assert sub == {}
    assert json.load(open(tmp_path / "results_test_s" / "submission.json"))[0] == {"image_id": 0, "caption": "a dog"}
    with pytest.raises(ValueError, match="twice"):
        E.validate_cap(m, cap + cap[:1], "cap%tv", refs, scorer="host")
    # a CaptionMetrics without a tokenizer is used through a copy: the caller's object still refuses strings; a wrapped model is unwrapped
    plain = capeval.CaptionMetrics({i: [capeval.simple_tokenize(r) if isinstance(r, str) else r for r in rs] for i, rs in refs.items()})
    assert E.validate_cap(m, cap, "cap%tv", plain, scorer="host") == {"tv": c["tv"]} and plain.tokenize is None
    with pytest.raises(TypeError):
        plain.score([0], ["a dog"])
    wrapped = type("Wrapper", (), {"module": _StubModel({"coco_submit": True}), "eval": lambda self: self.module.eval(),
                                   "__call__": lambda self, *a, **k: self.module(*a, **k)})()
    assert E.validate_cap(wrapped, named, "cap%tv", str(ann), scorer="host") == {}          # the submit switch of the wrapped model's options
    with pytest.raises(NotImplementedError):
        E.validate_single(m, [], "vqa%tv")
    with pytest.raises(ValueError):
        E.validate_single(m, cap, "cap%tv")                                    # no annotations, no loader.dataset.annfile
