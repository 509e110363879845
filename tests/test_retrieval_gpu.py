"""Retrieval evaluation on the GPU (csrc/retrieval.hip, valor_amd/evaluate.py retrieval_metrics / validate_ret) against the fixtures the
unmodified reference produced (tests/golden/ret_metric_*.pt, tools/make_ret_goldens.py) and against the CPU oracle end to end.

Without dual softmax the kernel compares the very fp32 values the reference sorts: ranks and dicts are EQUAL. With dual softmax the
device's exp differs from torch's: a query whose competitors all lie outside the band delta = 8 * e_ref (e_ref: the reference's own fp32
deviation from fp64, stored in the fixture) must have exactly its fp64 rank, an ambiguous one must land between the band counts
(tools/make_ret_goldens.py states the definitions). The small fixture has no ambiguous query, so its dict equals the reference's.

End to end the device's fine score matrix differs from the oracle's by the tolerance tests/test_evaluate_gpu.py grants that kernel path
(atol 2e-5, rtol 1e-5); through score * softmax(score / temp) with temp 0.07 and scores of a few tenths that is a relative change of at
most 2e-5 / |s| + 2 * 2e-5 / temp < 1e-3 of a value, so the batches are chosen such that the ORACLE has no competitor within E2E_BAND =
1e-3 of a ground truth (asserted), and then the logs must be equal."""
import dataclasses
import os
import random
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_ret_goldens as G  # noqa: E402

pytestmark = pytest.mark.gpu
E2E_BAND = 1e-3
OPTS = {"dropout": 0.0, "dual_softmax": True, "evaluate_ret_text": True}


def _case(name):
    fix = torch.load(os.path.join(ROOT, "tests", "golden", f"ret_metric_{name}.pt"), weights_only=False)
    score, ids, ids_txt = G.make_case(**G.CASES[name])
    assert G.checksum(score) == fix["checksum"], "the seeded matrix is not the one the fixture was made from"
    return fix, score, ids, ids_txt


def _device_ranks(score, ids, ids_txt, dev, **kw):
    from valor_amd.evaluate import _gt_columns, retrieval_ranks
    gt, ptr, rows = _gt_columns(ids, ids_txt, True)
    rf, rb = retrieval_ranks(score.to(dev), gt, ptr, rows, **kw)
    torch.cuda.synchronize()
    return rf.cpu(), rb.cpu()


@pytest.mark.parametrize("name", ["small", "large"])
def test_ranks_and_log_equal_the_reference_without_dual_softmax(dev, name):
    from valor_amd.evaluate import retrieval_metrics
    fix, score, ids, ids_txt = _case(name)
    rf, rb = _device_ranks(score, ids, ids_txt, dev)
    assert torch.equal(rf, fix["ranks"][False]["forward"]) and torch.equal(rb, fix["ranks"][False]["backward"])
    for text in (False, True):
        assert retrieval_metrics(score.to(dev), ids, ids_txt, text_direction=text) == fix["eval_log"][(False, text)]


@pytest.mark.parametrize("name", ["small", "large"])
def test_dual_softmax_ranks_within_the_band(dev, name):
    from valor_amd.evaluate import retrieval_metrics
    fix, score, ids, ids_txt = _case(name)
    delta = G.BAND_FACTOR * fix["e_ref"]
    bands = G.band_counts(score, ids, ids_txt, fix["temp"], True, delta)
    rf, rb = _device_ranks(score, ids, ids_txt, dev, dual_softmax=True, temp=fix["temp"])
    for k, got in (("forward", rf), ("backward", rb)):
        rank, lo, hi = bands[k]
        amb = lo != hi
        share = float(amb.double().mean())
        wrong = int((got.long() != rank)[~amb].sum())
        outside = int(((got.long() < lo) | (got.long() > hi)).sum())
        print(f"{name} {k}: delta {delta:.3g}, ambiguous share {share:.4f}, mismatches on unambiguous queries {wrong}, outside the band {outside}, "
              f"differing from fp64 at all {int((got.long() != rank).sum())}")
        assert share <= G.CASES[name]["max_ambiguous"]
        assert wrong == 0 and outside == 0
    if name == "small":
        for text in (False, True):
            assert retrieval_metrics(score.to(dev), ids, ids_txt, dual_softmax=True, temp=fix["temp"], text_direction=text) == fix["eval_log"][(True, text)]


@pytest.mark.parametrize("dual", [False, True])
def test_padded_rows_take_the_vector_path_with_a_tail(dev, dual):
    """the small matrix (50 columns: scalar loads) inside a [150, 52] buffer (16-byte loads, two masked tail columns holding +inf)"""
    fix, score, ids, ids_txt = _case("small")
    from valor_amd.evaluate import _gt_columns, retrieval_ranks
    buf = torch.full((150, 52), float("inf"), device=dev)
    buf[:, :50] = score.to(dev)
    gt, ptr, rows = _gt_columns(ids, ids_txt, True)
    rf, rb = retrieval_ranks(buf[:, :50], gt, ptr, rows, dual_softmax=dual, temp=fix["temp"])
    assert torch.equal(rf.cpu(), fix["ranks"][dual]["forward"]) and torch.equal(rb.cpu(), fix["ranks"][dual]["backward"])


def test_ties_rank_in_index_order_and_nan_stays_in_range(dev):
    from valor_amd.evaluate import retrieval_ranks
    s = torch.zeros((5, 6), device=dev)                       # every value ties: the rank is the number of lower indices
    gt = [3, 0, 5, 2, 2]
    rf, rb = retrieval_ranks(s, gt, [0, 1, 1, 3, 4, 4, 5], [1, 3, 4, 0, 2])
    assert rf.tolist() == [3, 0, 5, 2, 2] and rb.tolist() == [1, -1, 3, 0, -1, 2]
    g = torch.Generator().manual_seed(0)
    s = torch.randn((70, 300), generator=g)
    s[torch.rand((70, 300), generator=g) < 0.2] = float("nan")
    gt = torch.randint(0, 300, (70,), generator=g)
    order = torch.argsort(gt, stable=True)
    ptr = torch.cat((torch.zeros(1, dtype=torch.long), torch.bincount(gt, minlength=300).cumsum(0)))
    for dual in (False, True):
        rf, rb = retrieval_ranks(s.to(dev), gt.tolist(), ptr.tolist(), order.tolist(), dual_softmax=dual, temp=0.07)
        assert int(rf.min()) >= 0 and int(rf.max()) < 300 and int(rb.min()) >= -1 and int(rb.max()) < 70
    x = s.clone()
    t = x[torch.arange(70), gt][:, None]
    want = ((x > t) | ((x == t) & (torch.arange(300)[None] < gt[:, None]))).sum(1)        # a NaN compares as not greater
    rf, _ = retrieval_ranks(s.to(dev), gt.tolist())
    assert torch.equal(rf.cpu().long(), want)


# ------------------------------------------------------------------ end to end: validate_ret against the oracle
def _batches(spec, captions, seed0, n_batches=3, clips=4, q=False):
    from valor_amd import synth
    out = []
    for i in range(n_batches):
        b = synth.make_batch(spec, batch=clips, frames=2, audio_slices=1, txt_len=32, seed=seed0 + i, bf16_exact=q)
        b["ids"] = [f"v{clips * i + j}" for j in range(clips)]
        if captions > 1:
            t = synth.make_batch(spec, batch=clips * captions, frames=2, audio_slices=1, txt_len=32, seed=seed0 + 100 + i, bf16_exact=q)
            # the oracle sizes the decoder inputs by the text rows even where no decoder runs: it gets the clips and the captions as two
            # batches of matching row counts (the features of one modality do not depend on the others)
            b["_oracle_parts"] = (dict(b), t)
            b["txt_tokens"] = t["txt_tokens"]
        b["ids_txt"] = [b["ids"][j // captions] for j in range(clips * captions)]
        out.append(b)
    return out


def _oracle_log(spec, sd, batches, task, dual=True, text=True):
    """the reference's validate_ret restated on the CPU oracle: features of forward_ret(compute_loss=False), Oracle.compute_fine_matrix /
    matmul, fp64 stable ranks (tools/make_ret_goldens.py), the host metric pinned by the fixtures. Asserts that no query is ambiguous."""
    import valor_oracle as VO
    from valor_amd import synth
    orc = VO.Oracle(spec, sd, vocab_tokens=synth.synthetic_vocab(spec.vocab))
    groups = task.split("%")[1:]
    feats = {"feat_t": [], "feat_v": [], "feat_a": [], "txt_tokens": []}
    with torch.no_grad():
        for b in batches:
            if "_oracle_parts" in b:
                clips, caps = (orc.forward_ret(part, task, compute_loss=False) for part in b["_oracle_parts"])
                ev = dict(feat_v=clips["feat_v"], feat_a=clips["feat_a"], feat_t=caps["feat_t"], txt_tokens=caps["txt_tokens"])
            else:
                ev = orc.forward_ret(b, task, compute_loss=False)
            for k in feats:
                feats[k].append(ev[k])
        ft, fv, fa, tok = (torch.cat(feats[k], 0) if feats[k][0] is not None else None for k in feats)
    ids = [x for b in batches for x in b["ids"]]
    ids_txt = [x for b in batches for x in b["ids_txt"]]
    temp = float(1.0 / sd["clip_model.logit_scale"].exp()) if spec.video_encoder == "clip" else float(sd["contra_temp"])
    fw, cfm = orc.fine_weight, orc.compute_fine_matrix
    ones = lambda f: torch.ones(f.shape[:2])
    mats = {}
    with torch.no_grad():
        if spec.contra_type == "coarse":
            if "tv" in groups:
                mats["t_v"] = (ft @ fv.t(), "video", "txt")
            if "tva" in groups:
                if spec.late_fusion:
                    sm = ft @ fv.t() + ft @ fa.t()
                else:
                    fva = torch.nn.functional.normalize(torch.nn.functional.linear(torch.cat((fv, fa), -1), sd["va_fusion.weight"], sd["va_fusion.bias"]), dim=-1)
                    sm = ft @ fva.t()
                mats["t_va"] = (sm, "video", "txt")
            if "ta" in groups:
                mats["t_a"] = (ft @ fa.t(), "audio", "txt")
        else:
            mt = (tok != 0).long()
            if "tv" in groups:
                mats["t_v"] = (cfm(ft, fv, mt, ones(fv).long(), fw("text", ft), fw("video", fv)), "video", "txt")
            if "tva" in groups:
                if spec.late_fusion:
                    sm = cfm(ft, fv, mt, ones(fv).long(), ones(ft), ones(fv)) + cfm(ft, fa, mt, ones(fa).long(), ones(ft), ones(fa))
                else:
                    fva = torch.cat((fv, fa), 1)
                    sm = cfm(ft, fva, mt, ones(fva).long(), fw("text", ft), torch.cat((fw("video", fv), fw("audio", fa)), 1))
                mats["t_va"] = (sm, "video", "txt")
            if "ta" in groups:
                mats["t_a"] = (cfm(ft, fa, mt, ones(fa).long(), fw("text", ft), fw("audio", fa)), "audio", "txt")
            if "va" in groups:
                mats["v_a"] = (cfm(fv, fa, ones(fv).long(), ones(fa).long(), fw("video", fv), fw("audio", fa)), "audio", "video")
            if "vta" in groups:
                mats["v_ta"] = (cfm(fv, torch.cat((ft, fa), 1), ones(fv).long(), torch.cat((mt, ones(fa).long()), 1), fw("video", fv),
                                    torch.cat((fw("text", ft), fw("audio", fa)), 1)), "ta", "video")
            if "atv" in groups:
                mats["a_tv"] = (cfm(fa, torch.cat((ft, fv), 1), ones(fa).long(), torch.cat((mt, ones(fv).long()), 1), fw("audio", fa),
                                    torch.cat((fw("text", ft), fw("video", fv)), 1)), "tv", "audio")
    log = {}
    for key, (sm, f, b) in mats.items():
        bands = G.band_counts(sm.float(), ids, ids_txt, temp, dual, E2E_BAND)
        for k, (rank, lo, hi) in bands.items():
            assert torch.equal(lo, hi), f"{key} {k}: the oracle has an ambiguous query at {E2E_BAND}; pick other batch seeds"
        d = G.host_metrics(bands["forward"][0], "forward")
        if text:
            d.update(G.host_metrics(bands["backward"][0], "backward"))
        log[key] = {k.replace("forward", f).replace("backward", b): v for k, v in d.items()}
    return log


# (contra_type, late_fusion, captions per clip, task, batch seed). The reference itself cannot score va / vta / atv with several captions per
# clip (test.py:364 concatenates text and audio features along the token axis, :720 asserts len(ids_txt) rows): those groups run with one.
E2E = [("fine", False, 2, "ret%tv%tva%ta", 70), ("fine", True, 2, "ret%tv%tva%ta", 70), ("fine", False, 1, "ret%tv%tva%ta%va%vta%atv", 140),
       ("fine", True, 1, "ret%tv%tva%ta%va%vta%atv", 140), ("coarse", False, 2, "ret%tv%tva%ta", 30), ("coarse", True, 2, "ret%tv%tva%ta", 30)]


@pytest.mark.parametrize("contra,late,captions,task,seed0", E2E)
def test_validate_ret_matches_the_oracle(dev, contra, late, captions, task, seed0):
    from valor_amd import synth
    from valor_amd.evaluate import validate_ret
    from valor_amd.model.valor import VALOR
    spec = dataclasses.replace(synth.tiny_spec(), contra_type=contra, late_fusion=late)
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    batches = _batches(spec, captions, seed0)
    want = _oracle_log(spec, sd, batches, task)
    model = VALOR(dict(OPTS), spec=spec, dtype=torch.float32, device=dev)
    model.load_state_dict(sd, strict=True)
    got = validate_ret(model, batches, task)
    keys = {"tv": "t_v", "tva": "t_va", "ta": "t_a", "va": "v_a", "vta": "v_ta", "atv": "a_tv"}
    assert set(got) == {keys[g] for g in task.split("%")[1:]}
    assert set(got["t_v"]) == {f"{p}_{m}" for p in ("video", "txt") for m in ("recall", "ravg", "medianR", "meanR")}
    assert got == want, (got, want)


def test_bf16_model_scores_through_the_fused_kernel(dev):
    """bf16 features: valor_fine_fused_fwd in scores-only mode (chunked over A rows here) against the fp32-buffer path on the SAME bf16
    features at the tolerance tests/test_contrastive_fused_gpu.py uses for that pair (atol 1e-6); ranks equal on unambiguous queries."""
    from valor_amd import evaluate as E, synth
    from valor_amd.evaluate import _gt_columns, compute_fine_matrix, fine_score_matrix, retrieval_ranks, validate_ret
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05, bf16_exact=True)
    batches = _batches(spec, 2, 10, q=True)
    model = VALOR(dict(OPTS), spec=spec, dtype=torch.bfloat16, device=dev)
    model.load_state_dict(sd, strict=True)
    model.eval()
    task = "ret%tv%tva%ta"
    evs = [model(b, task=task, compute_loss=False) for b in batches]
    ft, fv = (torch.cat([e[k] for e in evs], 0).contiguous() for k in ("feat_t", "feat_v"))
    assert ft.dtype == torch.bfloat16
    tok = torch.cat([e["txt_tokens"].to(dev) for e in evs], 0)
    mt, mv = (tok != 0).float(), torch.ones(fv.shape[:2], device=dev)
    wt, wv = E._fine_weights(model, "text", ft), E._fine_weights(model, "video", fv)
    wide = compute_fine_matrix(ft, fv, mt, mv, wt, wv)
    fused = fine_score_matrix(ft, fv, mt, mv, wt, wv)
    old, E._FUSED_BYTES = E._FUSED_BYTES, 5 * ft.shape[1] * ft.shape[2] * 2 + 1          # five texts per launch: the chunking path
    try:
        chunked = fine_score_matrix(ft, fv, mt, mv, wt, wv)
    finally:
        E._FUSED_BYTES = old
    assert torch.equal(chunked, fused)
    print("fused vs fp32-buffer path, max abs difference", float((fused - wide).abs().max()))
    assert torch.allclose(fused, wide, atol=1e-6)
    ids = [x for b in batches for x in b["ids"]]
    ids_txt = [x for b in batches for x in b["ids_txt"]]
    temp = E.retrieval_temperature(model)
    bands = G.band_counts(wide.cpu(), ids, ids_txt, temp, True, E2E_BAND)
    gt, ptr, rows = _gt_columns(ids, ids_txt, True)
    rf, rb = retrieval_ranks(fused, gt, ptr, rows, dual_softmax=True, temp=temp)
    for k, got in (("forward", rf), ("backward", rb)):
        rank, lo, hi = bands[k]
        ok = lo == hi
        assert torch.equal(got.cpu().long()[ok], rank[ok]) and bool(((got.cpu().long() >= lo) & (got.cpu().long() <= hi)).all())
    log = validate_ret(model, batches, task)
    assert set(log) == {"t_v", "t_va", "t_a"} and len(log["t_v"]) == 8


def _ret_shards():
    from valor_amd import synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    bs = _batches(spec, 2, 10)
    return spec, sd, [[bs[0], bs[2]], [bs[1]]]


def _ret_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        spec, sd, shards = _ret_shards()
        from valor_amd.evaluate import validate_ret
        from valor_amd.model.valor import VALOR
        torch.cuda.set_device(0)
        model = VALOR(dict(OPTS), spec=spec, dtype=torch.float32, device="cuda:0")
        model.load_state_dict(sd, strict=True)
        torch.save(validate_ret(model, shards[rank], "ret%tv%tva%ta"), os.path.join(outdir, f"ret{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_validate_ret_gathers_the_ranks_shards(dev, tmp_path):
    """two ranks (gloo, one GPU) with unequal shards return, each, the log one process returns for the shards in rank order"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_ret_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    logs = [torch.load(tmp_path / f"ret{r}.pt", weights_only=False) for r in range(2)]
    spec, sd, shards = _ret_shards()
    from valor_amd.evaluate import validate_ret
    from valor_amd.model.valor import VALOR
    model = VALOR(dict(OPTS), spec=spec, dtype=torch.float32, device=dev)
    model.load_state_dict(sd, strict=True)
    one = validate_ret(model, [b for shard in shards for b in shard], "ret%tv%tva%ta")
    assert set(one) == {"t_v", "t_va", "t_a"} and "txt_recall" in one["t_v"]
    assert logs[0] == one and logs[1] == one, (logs, one)
