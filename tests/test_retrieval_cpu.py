"""Retrieval evaluation, host side (valor_amd/evaluate.py retrieval_metrics / validate_ret, csrc/retrieval.hip): ground-truth columns,
the two ValueErrors, metric formatting from the golden ranks to the reference's eval_log (tests/golden/ret_metric_*.pt, written by
tools/make_ret_goldens.py from the unmodified reference), the ABI entries and their argument checks without a GPU."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_ret_goldens as G  # noqa: E402


def _fixture(name):
    return torch.load(os.path.join(ROOT, "tests", "golden", f"ret_metric_{name}.pt"), weights_only=False)


def test_ground_truth_columns_first_occurrence_and_csr():
    from valor_amd.evaluate import _gt_columns
    ids = ["a", "b", "a", "c"]                       # column 2 repeats clip "a": ids.index picks column 0
    ids_txt = ["c", "a", "b", "a", "c"]
    gt, ptr, rows = _gt_columns(ids, ids_txt, True)
    assert gt == [ids.index(t) for t in ids_txt] == [3, 0, 1, 0, 3]
    assert ptr == [0, 2, 3, 5, 7] and rows == [1, 3, 2, 1, 3, 0, 4]      # the repeated column shares the texts of its clip (test.py:746-748)
    assert _gt_columns(ids, ids_txt, False)[1:] == (None, None)


def test_value_errors_where_the_reference_raises():
    from valor_amd.evaluate import _gt_columns, retrieval_metrics
    with pytest.raises(ValueError, match="not in ids"):
        _gt_columns(["a", "b"], ["a", "zzz"], False)
    with pytest.raises(ValueError, match="no text"):
        _gt_columns(["a", "b"], ["a", "a"], True)
    assert _gt_columns(["a", "b"], ["a", "a"], False)[0] == [0, 0]        # fine without the text direction
    with pytest.raises(ValueError, match="score matrix"):
        retrieval_metrics(torch.zeros(3, 2), ["a", "b"], ["a", "b"])


@pytest.mark.parametrize("name", ["small", "large"])
def test_metric_formatting_from_golden_ranks(name):
    """fp64 stable ranks -> exactly the reference's eval_log without dual softmax (it sorts the same fp32 values); with dual softmax
    on the small fixture too (no ambiguous query there)"""
    from valor_amd.evaluate import _metrics_from_ranks
    fix = _fixture(name)
    for dual in ((False, True) if name == "small" else (False,)):
        r = fix["ranks"][dual]
        log = dict(_metrics_from_ranks(r["forward"], "forward"), **_metrics_from_ranks(r["backward"], "backward"))
        assert log == fix["eval_log"][(dual, True)]
        assert {k: v for k, v in log.items() if k.startswith("forward")} == fix["eval_log"][(dual, False)]
    assert isinstance(log["forward_medianR"], float) and isinstance(log["forward_recall"], str)


def test_median_is_the_lower_middle_element():
    from valor_amd.evaluate import _metrics_from_ranks
    assert _metrics_from_ranks(torch.tensor([0, 3, 1, 10], dtype=torch.int32), "forward")["forward_medianR"] == 2.0


def test_small_fixture_is_the_seeded_matrix_and_meets_its_caps():
    fix = _fixture("small")
    score, ids, ids_txt = G.make_case(**G.CASES["small"])
    assert torch.equal(score, fix["score"]) and ids == fix["ids"] and ids_txt == fix["ids_txt"] and G.checksum(score) == fix["checksum"]
    assert score.shape == (150, 50) and len(set(ids)) == 48
    assert not G.has_exact_tie(score, ids, ids_txt)
    b = G.band_counts(score, ids, ids_txt, fix["temp"], True, G.BAND_FACTOR * fix["e_ref"])
    for k, (rank, lo, hi) in b.items():
        assert torch.equal(lo, hi) and torch.equal(rank.to(torch.int32), fix["ranks"][True][k])
    assert 0 < fix["e_ref"] < 1e-4 and max(_fixture("large")["ambiguous_share"].values()) <= 0.05


def test_abi_entries_and_argument_validation_without_gpu():
    from valor_amd import lib
    so = lib.load()
    assert {"valor_retrieval_ranks", "valor_retrieval_workspace_bytes"} <= set(lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "valor_hip.h")).read()
    assert "int valor_retrieval_ranks(" in hdr and "int valor_retrieval_workspace_bytes(" in hdr and "TIE RULE" in hdr
    n = ctypes.c_int64(-1)
    assert so.valor_retrieval_workspace_bytes(0, 7, ctypes.byref(n)) == 0 and n.value == 0
    assert so.valor_retrieval_workspace_bytes(25000, 5000, ctypes.byref(n)) == 0
    assert 0 < n.value < 25000 * 5000 * 4 // 8            # column partials, no [Nt, Nv] temporary
    assert so.valor_retrieval_workspace_bytes(4, 4, None) == -1 and so.valor_retrieval_workspace_bytes(-1, 4, ctypes.byref(n)) == -1
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    so.valor_retrieval_workspace_bytes(8, 8, ctypes.byref(n))
    base = dict(st=None, score=p, ld=8, gt=p, ptr=p, rows=p, nnz=8, k=1.0, dual=0, lr=None, lc=None, rf=p, rb=p, ws=p, wsb=n.value, Nt=8, Nv=8)
    call = lambda **kw: so.valor_retrieval_ranks(*{**base, **kw}.values())
    assert call(Nt=0) == 0 and call(Nv=0) == 0 and call(Nt=0, score=None) == 0          # zero sizes: no-op
    for bad in (dict(score=None), dict(gt=None), dict(rf=None), dict(ws=None), dict(ptr=None), dict(rows=None), dict(nnz=-1), dict(score=p + 2), dict(gt=p + 1),
                dict(rf=p + 2), dict(rb=p + 3), dict(ws=p + 4), dict(ld=7), dict(wsb=n.value - 1), dict(dual=1, k=0.0), dict(dual=1, k=float("nan")),
                dict(lc=p + 1, dual=1)):
        assert call(**bad) == -1, bad


@pytest.mark.skipif(not __import__("ref_harness").available(), reason="the reference tree is not present")
def test_fixtures_regenerate_from_the_reference():
    """tools/make_ret_goldens.py against the unmodified reference gives the committed fixtures (a subprocess: the harness patches torch)"""
    import subprocess
    code = ("import sys, torch; sys.path.insert(0, 'tools'); import make_ret_goldens as G\n"
            "for n in G.CASES:\n"
            "    new = G.generate(n); old = torch.load(f'tests/golden/ret_metric_{n}.pt', weights_only=False)\n"
            "    assert new.keys() == old.keys(), n\n"
            "    for k in new:\n"
            "        if k == 'ranks':\n"
            "            assert all(torch.equal(new[k][d][s], old[k][d][s]) for d in (False, True) for s in ('forward', 'backward')), (n, k)\n"
            "        elif k == 'score':\n"
            "            assert torch.equal(new[k], old[k])\n"
            "        else:\n"
            "            assert new[k] == old[k], (n, k, new[k], old[k])\n"
            "print('same')\n")
    env = {k: v for k, v in os.environ.items() if k not in ("MASTER_PORT", "MASTER_ADDR", "RANK", "WORLD_SIZE")}      # the child opens its own one-rank group
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "same" in r.stdout, r.stderr[-2000:]
