"""Evaluation of a pretraining run (first slice): test.py::validate_pt -- masked-token accuracy of the caption /
mlm passes (test.py:462-533, the "argmax token ids" of the north star) and the in-batch retrieval recall from the fine-grained
score matrices of the whole validation set (test.py:534-660, 714-774) -- on the same HIP kernels as training: the model's
compute_loss=False branch produces scores / features, the all-pairs similarity is the bf16 / fp32 GEMM and the per-pair reduction
is valor_fine_scores (rectangular, forward only). The reference's slicing of large sets (pretrain.py:178-186: rows of A in slices of
100 once B has more than 1200 items) is kept, with the slice size a parameter (288 GB of HBM hold far larger tiles)."""
import math

import torch

from . import kernels as K
from . import lib, ops
from .lib import ACT_RELU


def _fine_weights(model, name, feat):
    """fine_weight_mapper[name](feat).squeeze(2) (pretrain.py:104-116), no grad"""
    P = model.P
    h = ops.linear(feat, P[f"{name}_fine_weight.0.weight"], P[f"{name}_fine_weight.0.bias"], ACT_RELU)
    return ops.rowdot(h, P[f"{name}_fine_weight.2.weight"], P[f"{name}_fine_weight.2.bias"]).float().squeeze(-1).contiguous()


def _scores_gemm(featA, featB, maskA, maskB, wA, wB, out=None):
    """[NA, NB] fine scores through the token-similarity GEMM + valor_fine_scores; wA / wB are the SOFTMAXED token weights (contiguous
    fp32, like the masks). `out`: a dense fp32 [NA, NB] tensor to fill. Shared by compute_fine_matrix and search.RetrievalIndex."""
    NA, T, D = featA.shape
    NB, Nv = featB.shape[:2]
    f32 = dict(dtype=torch.float32, device=featA.device)
    fa, fb = featA.contiguous().view(NA * T, D), featB.contiguous().view(NB * Nv, D)
    ldS = (NB * Nv + 7) // 8 * 8
    S = torch.empty((NA * T, ldS), **f32)
    K.gemm(fa, fb, out=S[:, :NB * Nv], out_dtype=torch.float32, splitk=False)
    score = torch.empty((NA, NB), **f32) if out is None else out
    lib.call("valor_fine_scores", K._stream(), S.data_ptr(), ldS, maskA.data_ptr(), maskB.data_ptr(), wA.data_ptr(), wB.data_ptr(), score.data_ptr(),
             NA, NB, T, Nv)
    return score


def _fine_matrix_slice(featA, featB, maskA, maskB, wA_raw, wB_raw):
    NA, T = featA.shape[:2]
    NB, Nv = featB.shape[:2]
    f32 = dict(dtype=torch.float32, device=featA.device)
    wA, wB = torch.empty((NA, T), **f32), torch.empty((NB, Nv), **f32)
    st = K._stream()
    lib.call("valor_fine_weight_softmax", st, wA_raw.data_ptr(), maskA.data_ptr(), wA.data_ptr(), NA, T)
    lib.call("valor_fine_weight_softmax", st, wB_raw.data_ptr(), maskB.data_ptr(), wB.data_ptr(), NB, Nv)
    return _scores_gemm(featA, featB, maskA, maskB, wA, wB)


@torch.no_grad()
def compute_fine_matrix(featA, featB, maskA, maskB, weightA, weightB, slice_rows=100, slice_above=1200):
    """VALOR.compute_fine_matrix (pretrain.py:178-189): [NA, NB] scores; rows of A in slices once B exceeds `slice_above` items."""
    maskA, maskB = maskA.float().contiguous(), maskB.float().contiguous()
    weightA, weightB = weightA.float().contiguous(), weightB.float().contiguous()
    if featB.shape[0] > slice_above:
        out = []
        for i in range(math.ceil(featA.shape[0] / slice_rows)):
            sl = slice(i * slice_rows, (i + 1) * slice_rows)
            out.append(_fine_matrix_slice(featA[sl], featB, maskA[sl], maskB, weightA[sl], weightB))
        return torch.cat(out, dim=0)
    return _fine_matrix_slice(featA, featB, maskA, maskB, weightA, weightB)


def compute_metric_ret(score_matrix, ids, ids_txt):
    """test.py:714-774 without dual softmax / text-retrieval direction: rank of the ground-truth video for every text."""
    order = score_matrix.sort(dim=-1, descending=True)[1].tolist()
    rank = torch.tensor([order[i].index(ids.index(ids_txt[i])) for i in range(len(ids_txt))], dtype=torch.float32)
    r1, r5, r10 = [(rank < k).sum().item() / len(ids_txt) for k in (1, 5, 10)]
    return {"forward_recall": f"{round(r1 * 100, 1)}/{round(r5 * 100, 1)}/{round(r10 * 100, 1)}", "forward_ravg": round((r1 + r5 + r10) / 3 * 100, 1),
            "forward_medianR": torch.median(rank).item() + 1, "forward_meanR": torch.mean(rank).item() + 1}


@torch.no_grad()
def validate_pt(model, loader, task):
    """test.py::validate_pt (:404-665): `loader` yields THIS RANK's batches of valor_collate (+ 'ids_txt'); returns the val_log dict
    (caption_acc_* / mlm_acc_* rounded to 2 digits, t2v / t2va / t2a forward recall strings).
    Under data parallelism (torch.distributed initialised, world > 1) every rank scores its shard and the reference's collectives run:
    ids / ids_txt and the hit / word counters through all_gather_list (test.py:275-276, 496-518), features and tokens through
    ddp_allgather (:279-290; per-rank sizes may differ). The recall is computed on the gathered set; the reference does that on rank 0
    only and leaves the other ranks' val_log without it -- here every rank returns the full log.
    Kept quirk: the mlm hit counters are selected by the CAPTION group list (test.py:484-492)."""
    from . import dist as vdist
    model.eval()
    mlm_task, caption_task, contra_task = [], [], []
    for i in task.split("_"):
        if "mlm" in i:
            mlm_task = i.split("%")[1:]
        elif "caption" in i:
            caption_task = i.split("%")[1:]
        elif "contra" in i:
            contra_task = i.split("%")[1:]
    n_word = {"caption": 0, "mlm": 0}
    hits = {}
    feats = {"feat_t": [], "feat_v": [], "feat_a": [], "txt_tokens": []}
    ids, ids_txt = [], []
    for batch in loader:
        ev = model(batch, task=task, compute_loss=False)
        if contra_task:
            for k in feats:
                feats[k].append(ev[k])
            ids += list(batch["ids"])
            ids_txt += list(batch.get("ids_txt", batch["ids"]))
        for tag, groups in (("caption", caption_task), ("mlm", mlm_task)):
            if not groups:
                continue
            lab = ev[f"txt_labels_{tag}"]
            lab = lab[lab != -1].to(model.device)
            n_word[tag] += lab.numel()
            for g in ("tva", "tv", "ta"):
                if g in caption_task and f"{tag}_scores_{g}" in ev:
                    hits[f"{tag}_{g}"] = hits.get(f"{tag}_{g}", 0) + int((ev[f"{tag}_scores_{g}"].max(dim=-1)[1] == lab).sum().item())
    if vdist.is_dist():
        # test.py:496-518: sum(all_gather_list(counter)) per counter -- one object collective for all of them here
        every = vdist.all_gather_list((n_word, hits))
        n_word = {k: sum(nw[k] for nw, _ in every) for k in n_word}
        hits = {k: sum(h.get(k, 0) for _, h in every) for k in sorted({k for _, h in every for k in h})}
        if contra_task:
            ids = [j for part in vdist.all_gather_list(ids) for j in part]               # test.py:275-276
            ids_txt = [j for part in vdist.all_gather_list(ids_txt) for j in part]
            for k in feats:                                                              # test.py:279-290
                if feats[k] and feats[k][0] is not None:
                    feats[k] = [vdist.ddp_allgather(torch.cat([t.to(model.device) for t in feats[k]], dim=0))]
    val_log = {}
    for tag, groups in (("caption", caption_task), ("mlm", mlm_task)):
        for g in ("tva", "tv", "ta"):
            if g in groups and f"{tag}_{g}" in hits:
                val_log[f"{tag}_acc_{g}"] = round(hits[f"{tag}_{g}"] / n_word[tag], 2)
    if contra_task and model.spec.contra_type == "coarse":            # test.py:640-660: plain similarity matrices of the pooled features
        from . import kernels as K, ops
        cat = lambda k: torch.cat(feats[k], dim=0).contiguous() if feats[k] and feats[k][0] is not None else None
        ft, fv, fa = cat("feat_t"), cat("feat_v"), cat("feat_a")
        sim = lambda a, b: K.gemm(a, b, out_dtype=torch.float32)
        with torch.no_grad():
            if "tv" in contra_task:
                val_log["t2v_recall"] = compute_metric_ret(sim(ft, fv).cpu(), ids, ids_txt)["forward_recall"]
            if "tva" in contra_task:
                if model.spec.late_fusion:
                    sm = sim(ft, fv) + sim(ft, fa)
                else:
                    fva = ops.l2_normalize(ops.linear(torch.cat((fv, fa), dim=-1), model.P["va_fusion.weight"], model.P["va_fusion.bias"]))
                    sm = sim(ft, fva)
                val_log["t2va_recall"] = compute_metric_ret(sm.cpu(), ids, ids_txt)["forward_recall"]
            if "ta" in contra_task:
                val_log["t2a_recall"] = compute_metric_ret(sim(ft, fa).cpu(), ids, ids_txt)["forward_recall"]
        return val_log
    if contra_task:
        cat = lambda k: torch.cat(feats[k], dim=0) if feats[k] and feats[k][0] is not None else None
        ft, fv, fa = cat("feat_t"), cat("feat_v"), cat("feat_a")
        tok = torch.cat([t.to(model.device) for t in feats["txt_tokens"]], dim=0)
        maskA = (tok != 0).float()
        wt = _fine_weights(model, "text", ft)
        ones = lambda f: torch.ones(f.shape[:2], dtype=torch.float32, device=model.device)
        if "tv" in contra_task:
            val_log["t2v_recall"] = compute_metric_ret(compute_fine_matrix(ft, fv, maskA, ones(fv), wt, _fine_weights(model, "video", fv)).cpu(), ids, ids_txt)["forward_recall"]
        if "tva" in contra_task and model.spec.late_fusion:          # test.py:571-579: unit token weights, the tv and ta matrices summed
            sm = compute_fine_matrix(ft, fv, maskA, ones(fv), ones(ft), ones(fv)) + compute_fine_matrix(ft, fa, maskA, ones(fa), ones(ft), ones(fa))
            val_log["t2va_recall"] = compute_metric_ret(sm.cpu(), ids, ids_txt)["forward_recall"]
        elif "tva" in contra_task:
            fva = torch.cat((fv, fa), dim=1)
            wva = torch.cat((_fine_weights(model, "video", fv), _fine_weights(model, "audio", fa)), dim=1)
            val_log["t2va_recall"] = compute_metric_ret(compute_fine_matrix(ft, fva, maskA, ones(fva), wt, wva).cpu(), ids, ids_txt)["forward_recall"]
        if "ta" in contra_task:
            val_log["t2a_recall"] = compute_metric_ret(compute_fine_matrix(ft, fa, maskA, ones(fa), wt, _fine_weights(model, "audio", fa)).cpu(), ids, ids_txt)["forward_recall"]
    return val_log


# ------------------------------------------------------------------ retrieval evaluation (test.py:249-411 validate_ret, :685-775)
def _gt_columns(ids, ids_txt, text_direction):
    """gt_col[i] = ids.index(ids_txt[i]) (the first occurrence of a clip id wins) and, for the text direction, the texts of every clip
    as a CSR list. ValueError where the reference raises: a text whose clip is absent (ids.index), a clip without a text (min([]))."""
    first = {}
    for j, clip in enumerate(ids):
        first.setdefault(clip, j)
    gt_col = []
    for i, clip in enumerate(ids_txt):
        if clip not in first:
            raise ValueError(f"text {i}: clip id {clip!r} is not in ids")
        gt_col.append(first[clip])
    col_ptr = col_rows = None
    if text_direction:
        # test.py:746-748 compares ids_txt against ids[i] for EVERY column, so a duplicated clip id shares its texts with its copies
        by_clip = {}
        for i, clip in enumerate(ids_txt):
            by_clip.setdefault(clip, []).append(i)
        col_ptr, col_rows = [0], []
        for j, clip in enumerate(ids):
            rows = by_clip.get(clip)
            if not rows:
                raise ValueError(f"clip {j} ({clip!r}) has no text: the text-retrieval direction is undefined for it")
            col_rows += rows
            col_ptr.append(len(col_rows))
    return gt_col, col_ptr, col_rows


def _metrics_from_ranks(rank, prefix):
    """test.py:731-737, 760-774: fp32 ranks -> recall string, ravg, medianR (torch.median: the LOWER middle element), meanR"""
    n = rank.numel()
    rank = rank.to(torch.float32)
    r1, r5, r10 = [(rank < k).sum().item() / n for k in (1, 5, 10)]
    return {f"{prefix}_recall": f"{round(r1 * 100, 1)}/{round(r5 * 100, 1)}/{round(r10 * 100, 1)}",
            f"{prefix}_ravg": round((r1 + r5 + r10) / 3 * 100, 1),
            f"{prefix}_medianR": torch.median(rank).item() + 1,
            f"{prefix}_meanR": torch.mean(rank).item() + 1}


@torch.no_grad()
def retrieval_ranks(score, gt_col, col_ptr=None, col_rows=None, *, dual_softmax=False, temp=None):
    """valor_retrieval_ranks on a device fp32 matrix [Nt, Nv] (unit column stride): (rank_f int32 [Nt], rank_b int32 [Nv] or None) on
    the device; rank_b when the CSR lists are given. No [Nt, Nv] temporary: the workspace holds column partials of 1 / 16 of the matrix."""
    if score.dtype != torch.float32 or score.dim() != 2:
        raise ValueError("score: an fp32 [texts, clips] matrix")
    if score.stride(1) != 1 or score.stride(0) < score.shape[1]:
        score = score.contiguous()
    Nt, Nv = score.shape
    dev = score.device
    bwd = col_ptr is not None
    i32 = dict(dtype=torch.int32, device=dev)
    rank_f = torch.empty((Nt,), **i32)
    rank_b = torch.empty((Nv,), **i32) if bwd else None
    if Nt == 0 or Nv == 0:
        return rank_f, rank_b
    if dual_softmax and not (temp is not None and temp > 0):
        raise ValueError("dual_softmax needs the contrastive temperature")
    to_dev = lambda x: torch.as_tensor(x, dtype=torch.int32).to(dev)
    gt_col = to_dev(gt_col)
    if bwd:
        col_ptr, col_rows = to_dev(col_ptr), to_dev(col_rows)
    import ctypes
    nbytes = ctypes.c_int64()
    lib.call("valor_retrieval_workspace_bytes", Nt, Nv, ctypes.byref(nbytes))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    lib.call("valor_retrieval_ranks", K._stream(), p(score), score.stride(0), p(gt_col), p(col_ptr) if bwd else None, p(col_rows) if bwd else None, int(col_rows.numel()) if bwd else 0,
             1.0 / temp if dual_softmax else 0.0, int(bool(dual_softmax)), None, None, p(rank_f), p(rank_b), p(ws), nbytes.value, Nt, Nv)
    return rank_f, rank_b


@torch.no_grad()
def retrieval_metrics(score, ids, ids_txt, *, dual_softmax=False, temp=None, text_direction=False):
    """compute_metric_ret of test.py:714-775 with its two options (dual_softmax, evaluate_ret_text) on a DEVICE score matrix
    [len(ids_txt), len(ids)]: the ranks are counted on the device (valor_retrieval_ranks; ties in index order, the stable sort the
    reference leaves undefined), and only the two int32 rank vectors come back. Returns the reference's eval_log: forward_recall /
    _ravg / _medianR / _meanR and, with text_direction, the four backward_* keys."""
    if tuple(score.shape) != (len(ids_txt), len(ids)):
        raise ValueError(f"score matrix {tuple(score.shape)} against {len(ids_txt)} texts x {len(ids)} clips (test.py:720)")
    gt_col, col_ptr, col_rows = _gt_columns(ids, ids_txt, text_direction)
    rank_f, rank_b = retrieval_ranks(score, gt_col, col_ptr, col_rows, dual_softmax=dual_softmax, temp=temp)
    log = _metrics_from_ranks(rank_f.cpu(), "forward")
    if text_direction:
        log.update(_metrics_from_ranks(rank_b.cpu(), "backward"))
    return log


_FUSED_BYTES = 0x7f000000          # valor_fine_fused_fwd addresses each feature tensor with 32-bit byte offsets below this


@torch.no_grad()
def fine_score_matrix(featA, featB, maskA, maskB, weightA, weightB):
    """The [NA, NB] fine-grained score matrix of an evaluation. bf16 features: valor_fine_fused_fwd in its scores-only mode (the token
    similarities stay in registers: no fp32 [NA * T, NB * Nv] buffer), in chunks of A rows / B items where a tensor would pass the
    kernel's byte limit. fp32 features (parity mode): compute_fine_matrix. maskX [N, tokens], weightX raw token weights (softmaxed here)."""
    if featA.dtype != torch.bfloat16:
        return compute_fine_matrix(featA, featB, maskA, maskB, weightA, weightB)
    NA, T, D = featA.shape
    NB, Nv = featB.shape[:2]
    if T > 64 or Nv > 64 or D % 64:
        return compute_fine_matrix(featA, featB, maskA, maskB, weightA, weightB)
    dev = featA.device
    f32 = dict(dtype=torch.float32, device=dev)
    featA, featB = featA.contiguous(), featB.to(torch.bfloat16).contiguous()
    maskA, maskB = maskA.float().contiguous(), maskB.float().contiguous()
    st = K._stream()
    wA, wB = torch.empty((NA, T), **f32), torch.empty((NB, Nv), **f32)
    lib.call("valor_fine_weight_softmax", st, weightA.float().contiguous().data_ptr(), maskA.data_ptr(), wA.data_ptr(), NA, T)
    lib.call("valor_fine_weight_softmax", st, weightB.float().contiguous().data_ptr(), maskB.data_ptr(), wB.data_ptr(), NB, Nv)
    rb = max(1, min(NB, (_FUSED_BYTES - 1) // (Nv * D * 2)))
    cols = [_scores_fused(featA, featB[b0:b0 + rb], maskA, maskB[b0:b0 + rb], wA, wB[b0:b0 + rb]) for b0 in range(0, NB, rb)]
    return cols[0] if len(cols) == 1 else torch.cat(cols, dim=1)


def fused_scores_ok(featA, featB):
    """bf16 token features of a geometry valor_fine_fused_fwd takes (what fine_score_matrix asks before it chooses the kernel)"""
    return featA.dtype == torch.bfloat16 and featB.dtype == torch.bfloat16 and featA.shape[1] <= 64 and featB.shape[1] <= 64 and featA.shape[2] % 64 == 0


def _scores_fused(featA, featB, maskA, maskB, wA, wB, out=None):
    """[NA, nb] fine scores of contiguous bf16 features by valor_fine_fused_fwd in its scores-only mode, the A rows in pieces under the
    kernel's byte limit; featB (a slice of leading rows) must be under it already. wA / wB are the SOFTMAXED token weights (contiguous
    fp32, like the masks). `out`: a dense fp32 [NA, nb] tensor to fill. Shared by fine_score_matrix and search.RetrievalIndex."""
    NA, T, D = featA.shape
    nb, Nv = featB.shape[:2]
    st = K._stream()
    part = torch.empty((NA, nb), dtype=torch.float32, device=featA.device) if out is None else out
    ra = max(1, min(NA, (_FUSED_BYTES - 1) // (T * D * 2)))
    for a0 in range(0, NA, ra):
        na = min(ra, NA - a0)
        lib.call("valor_fine_fused_fwd", st, featA[a0:a0 + na].data_ptr(), featB.data_ptr(), maskA[a0:a0 + na].data_ptr(),
                 maskB.data_ptr(), wA[a0:a0 + na].data_ptr(), wB.data_ptr(), part[a0:a0 + na].data_ptr(),
                 None, None, None, None, na, nb, T, Nv, D)
    return part


def retrieval_temperature(model):
    """test.py:688-691: 1 / exp(logit_scale) for a CLIP video encoder, else contra_temp"""
    if model.spec.video_encoder == "clip":
        return float(1.0 / model.P["clip_model.logit_scale"].detach().float().exp())
    return float(model.P["contra_temp"].detach().float())


@torch.no_grad()
def validate_ret(model, loader, task):
    """test.py::validate_ret (:249-411): `loader` yields THIS RANK's batches of valor_collate (+ 'ids_txt': several captions per clip);
    `task` is 'ret%tva%tv...'. Returns the reference's nested val_log: val_log['t_v'] = {video_recall, video_ravg, video_medianR,
    video_meanR [, txt_*]}, 't_va', 't_a' (audio_* / txt_*), and for contra_type 'fine' also 'v_a', 'v_ta', 'a_tv'. dual_softmax and
    evaluate_ret_text come from the model's options. The features are gathered across ranks as in validate_pt, and as there every
    rank returns the full log (the reference fills it on rank 0 only). The score matrices stay on the device; the ranks are counted
    there (retrieval_metrics). The reference casts the gathered features to fp16 (:281-287); here they keep the model's dtype."""
    from . import dist as vdist
    from .model.valor import _opt
    model.eval()
    groups = task.split("%")[1:]
    feats = {"feat_t": [], "feat_v": [], "feat_a": [], "txt_tokens": []}
    ids, ids_txt = [], []
    for batch in loader:
        ev = model(batch, task=task, compute_loss=False)
        for k in feats:
            feats[k].append(ev[k])
        ids += list(batch["ids"])
        ids_txt += list(batch["ids_txt"] if batch.get("ids_txt") is not None else batch["ids"])
    if vdist.is_dist():
        ids = [j for part in vdist.all_gather_list(ids) for j in part]               # test.py:275-276
        ids_txt = [j for part in vdist.all_gather_list(ids_txt) for j in part]
        for k in feats:                                                              # test.py:279-290
            if feats[k] and feats[k][0] is not None:
                feats[k] = [vdist.ddp_allgather(torch.cat([t.to(model.device) for t in feats[k]], dim=0))]
    cat = lambda k: torch.cat([t.to(model.device) for t in feats[k]], dim=0).contiguous() if feats[k] and feats[k][0] is not None else None
    ft, fv, fa, tok = cat("feat_t"), cat("feat_v"), cat("feat_a"), cat("txt_tokens")
    kw = dict(dual_softmax=bool(_opt(model.opts, "dual_softmax", False)), temp=retrieval_temperature(model),
              text_direction=bool(_opt(model.opts, "evaluate_ret_text", False)))

    def metric(score, fwd, bwd):
        log = retrieval_metrics(score, ids, ids_txt, **kw)
        return {k.replace("forward", fwd).replace("backward", bwd): v for k, v in log.items()}

    val_log = {}
    if model.spec.contra_type == "coarse":                                           # test.py:383-406
        sim = lambda a, b: K.gemm(a, b, out_dtype=torch.float32)
        if "tv" in groups:
            val_log["t_v"] = metric(sim(ft, fv), "video", "txt")
        if "tva" in groups:
            if model.spec.late_fusion:
                sm = sim(ft, fv) + sim(ft, fa)
            else:
                fva = ops.l2_normalize(ops.linear(torch.cat((fv, fa), dim=-1), model.P["va_fusion.weight"], model.P["va_fusion.bias"]))
                sm = sim(ft, fva)
            val_log["t_va"] = metric(sm, "video", "txt")
        if "ta" in groups:
            val_log["t_a"] = metric(sim(ft, fa), "audio", "txt")
        return val_log
    ones = lambda f: torch.ones(f.shape[:2], dtype=torch.float32, device=model.device)
    mt = (tok != 0).float() if tok is not None else None
    fw = {}

    def weight(name, f):
        if name not in fw:
            fw[name] = _fine_weights(model, name, f)
        return fw[name]

    if "tv" in groups:                                                               # :296-305
        val_log["t_v"] = metric(fine_score_matrix(ft, fv, mt, ones(fv), weight("text", ft), weight("video", fv)), "video", "txt")
    if "tva" in groups:                                                              # :307-334
        if model.spec.late_fusion:
            sm = fine_score_matrix(ft, fv, mt, ones(fv), ones(ft), ones(fv)) + fine_score_matrix(ft, fa, mt, ones(fa), ones(ft), ones(fa))
        else:
            fva = torch.cat((fv, fa), dim=1)
            sm = fine_score_matrix(ft, fva, mt, ones(fva), weight("text", ft), torch.cat((weight("video", fv), weight("audio", fa)), dim=1))
        val_log["t_va"] = metric(sm, "video", "txt")
    if "ta" in groups:                                                               # :338-346
        val_log["t_a"] = metric(fine_score_matrix(ft, fa, mt, ones(fa), weight("text", ft), weight("audio", fa)), "audio", "txt")
    if "va" in groups:                                                               # :350-358
        val_log["v_a"] = metric(fine_score_matrix(fv, fa, ones(fv), ones(fa), weight("video", fv), weight("audio", fa)), "audio", "video")
    if "vta" in groups:                                                              # :361-370
        sm = fine_score_matrix(fv, torch.cat((ft, fa), dim=1), ones(fv), torch.cat((mt, ones(fa)), dim=1), weight("video", fv),
                               torch.cat((weight("text", ft), weight("audio", fa)), dim=1))
        val_log["v_ta"] = metric(sm, "ta", "video")
    if "atv" in groups:                                                              # :372-381
        sm = fine_score_matrix(fa, torch.cat((ft, fv), dim=1), ones(fa), torch.cat((mt, ones(fv)), dim=1), weight("audio", fa),
                               torch.cat((weight("text", ft), weight("video", fv)), dim=1))
        val_log["a_tv"] = metric(sm, "tv", "audio")
    return val_log


# ------------------------------------------------------------------ caption / QA evaluation (test.py:18-237, :781-788)
_GROUP_KEY = {"tv": "t_v", "tva": "t_va", "ta": "t_a"}


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _gathered(items):
    """test.py:101, :203: [i for j in all_gather_list(items) for i in j] -- this rank's list, or every rank's in rank order"""
    from . import dist as vdist
    return [i for part in vdist.all_gather_list(items) for i in part] if vdist.is_dist() else list(items)


def _unwrapped(model):
    """the VALOR under a DistributedDataParallel-style wrapper (the reference's get_model_attr)"""
    return getattr(model, "module", model)


def _decoder(model, decode):
    if decode is not None:
        return decode
    return _unwrapped(model).decode_sequence


def caption_metrics_for(annotations, tokenize=None, scorer="device", device="cuda:0"):
    """The scorer validate_cap uses, for a caller that keeps it across validation rounds (the device tables of the validation set are then
    built and uploaded once): annotations = the reference's annfile path, {clip id: [word list or caption string, ...]}, or a
    capeval.CaptionMetrics. scorer: 'device' (capeval.DeviceCaptionMetrics) or 'host' (capeval.CaptionMetrics)."""
    from . import capeval
    if scorer not in ("device", "host"):
        raise ValueError(f"scorer {scorer!r}: 'device' or 'host'")
    tok = tokenize if tokenize is not None else capeval.simple_tokenize
    if isinstance(annotations, capeval.DeviceCaptionMetrics):
        return annotations if scorer == "device" else annotations.host
    if isinstance(annotations, capeval.CaptionMetrics):
        host = annotations
    elif isinstance(annotations, (str, bytes)) or hasattr(annotations, "__fspath__"):
        host = capeval.CaptionMetrics.from_annotations(annotations, tokenize=tok)
    else:
        host = capeval.CaptionMetrics(annotations, tokenize=tok)
    if host.tokenize is None:                                                  # the hypotheses arrive as strings: a copy that splits them
        import copy                                                            # (shallow: the caller's scorer keeps refusing strings)
        host = copy.copy(host)
        host.tokenize = tok
    return capeval.DeviceCaptionMetrics(host, device=device) if scorer == "device" else host


def compute_metric_cap(results, metrics):
    """test.py:781-788 on [{'video_id', 'caption'}, ...]: the corpus metrics * 100 rounded to two decimals (no METEOR: capeval's docstring).
    The evaluated clips are the ids of the results (pycocoevalcap/eval.py:21); a clip with two results raises ValueError."""
    from . import capeval
    res = metrics.score([r["video_id"] for r in results], [r["caption"] for r in results])
    return capeval.rounded(res.corpus)


@torch.no_grad()
def validate_cap(model, loader, task, annotations, *, tokenize=None, decode=None, scorer="device", output_dir=None, global_step=0, dset_name=""):
    """test.py::validate_cap (:136-237): `loader` yields THIS RANK's batches; `task` is 'cap%tva%tv..'. Per batch the model's
    compute_loss=False branch generates, the sequences are decoded (model.decode_sequence, or `decode`: int [N, T] -> N strings), the
    result lists are gathered across ranks (all_gather_list) and every group is scored against `annotations` (caption_metrics_for) by
    capeval: on the device (`scorer='device'`, valor_caption_metrics) or on the host. Returns {'tva': {Bleu_1..4, ROUGE_L, CIDEr}, 'tv':
    .., 'ta': ..}, every value * 100 rounded to two decimals: the reference's val_log without METEOR (and with `tokenize`, default
    capeval.simple_tokenize, in the place of the PTB tokenizer; see capeval).
    With output_dir, rank 0 writes the reference's results_test_{dset_name}/step_{global_step}_{group}.json. coco_submit / nocaps_submit
    (group tv) and vatex_submit (group tva) from the model's options write submission.json in the reference's formats, and that group
    gets no metrics. Every rank returns the full log (as validate_pt / validate_ret; the reference fills 'ta' on rank 0 only): every
    rank scores the whole gathered set, so with raw annotations every rank also builds (host n-gram statistics and flat tables in
    Python: seconds at MSRVTT size) and uploads its own device tables on every call. Pass a scorer from
    caption_metrics_for and keep it across validation rounds: the tables are then built and uploaded once per rank."""
    import json
    import os
    from .model.valor import _opt
    core = _unwrapped(model)
    opts = getattr(core, "opts", None)
    coco, vatex, nocaps = (bool(_opt(opts, k, False)) for k in ("coco_submit", "vatex_submit", "nocaps_submit"))
    groups = [g for g in ("tva", "tv", "ta") if g in task.split("%")[1:]]      # the reference's order of evaluation (:202-233)
    dec = _decoder(model, decode)
    model.eval()
    results = {g: [] for g in groups}
    for batch in loader:
        ids = list(batch["ids"])
        ev = model(batch, task=task, compute_loss=False)
        for g in groups:
            sents = dec(ev["generated_sequences_" + _GROUP_KEY[g]])
            for i, s in zip(ids, sents):
                if g == "tv" and coco:
                    results[g].append({"image_id": int(str(i).split("_")[-1]), "caption": s})
                elif g == "tv" and nocaps:
                    results[g].append({"image_id": int(i), "caption": s})
                elif g == "tva" and vatex:
                    results[g].append({i: s})
                else:
                    results[g].append({"video_id": i, "caption": s})
    folder = None
    if output_dir is not None:
        folder = os.path.join(output_dir, f"results_test_{dset_name}")
        os.makedirs(folder, exist_ok=True)

    def dump(obj, name):
        if folder is not None and _rank() == 0:
            with open(os.path.join(folder, name), "w") as fh:
                json.dump(obj, fh)

    metrics = None
    val_log = {}
    for g in groups:
        res = _gathered(results[g])
        if g == "tva" and vatex:
            dump({k: v for r in res for k, v in r.items()}, "submission.json")
        elif g == "tv" and (coco or nocaps):
            dump(res, "submission.json")
        else:
            if metrics is None:
                metrics = caption_metrics_for(annotations, tokenize, scorer, device=str(getattr(core, "device", "cuda:0")))
            val_log[g] = compute_metric_cap(res, metrics)
            dump(res, f"step_{global_step}_{g}.json")
    return val_log


def _answer_strings(batch, dec):
    """the ground-truth answers of a QA batch as strings: batch['answers'], or the reference's eval schema (txt_tokens = the answer
    strings, test.py:71), or the training schema (txt_tokens['bert_tokens'] = [CLS] answer [SEP] rows), decoded like the predictions"""
    gt = batch.get("answers")
    if gt is None:
        gt = batch["txt_tokens"]
    if isinstance(gt, dict):
        return dec(gt["bert_tokens"][:, 1:])
    return list(gt)


def _answer_indices(batch):
    """the ground truth of a multiple-choice batch: integer answers in batch['answers'], or in txt_tokens (data/vqa.py:169-172)"""
    gt = batch.get("answers")
    if gt is None:
        gt = batch["txt_tokens"]
    if isinstance(gt, dict):
        raise ValueError("validate_qa(multiple_choice=True): the answers are token rows; multiple choice needs integer answers")
    gt = gt.reshape(-1).tolist() if torch.is_tensor(gt) else list(gt)
    if any(isinstance(a, (str, bytes)) or int(a) != a for a in gt):
        raise ValueError("validate_qa(multiple_choice=True): the answers must be integers (the index of the right choice)")
    return [int(a) for a in gt]


def _choice_sets(batch, n_questions):
    """the choices of a multiple-choice batch as a per-question AnswerSet: choice_tokens['bert_tokens'] holds the '[CLS] choice [SEP]' rows
    of all questions back to back (data/vqa.py:161-167), the same number for every question of the batch"""
    from . import decode as D
    rows = batch["choice_tokens"]["bert_tokens"]
    n = int(rows.shape[0])
    nums = batch.get("choice_nums")
    if nums is not None and len(set(int(c) for c in nums)) > 1:
        raise ValueError(f"validate_qa(multiple_choice=True): choice counts {list(nums)} differ inside a batch")
    if n_questions < 1 or n % n_questions or n == 0:
        raise ValueError(f"validate_qa(multiple_choice=True): {n} choice rows for {n_questions} questions: every question of a batch needs the "
                         "same number of choices")
    return D.AnswerSet.from_bert_rows(rows.cpu(), per_sample_counts=[n // n_questions] * n_questions)


@torch.no_grad()
def validate_qa(model, loader, task, *, decode=None, output_dir=None, global_step=0, dset_name="", candidates=None, multiple_choice=False,
                answer_ranking=None):
    """test.py::validate_qa (:44-130): the generated answers of every group, decoded to strings, are compared with the ground truth
    (exact string equality); answers and ground truth are gathered across ranks. Returns {'tv': {'accuracy': round(acc * 100, 2)}, ..}
    on every rank. With output_dir, rank 0 writes predict_answers/step{global_step}_gt.json, step{..}_tv_pred.json and the question_ids
    submission list step{..}_tv_pred_submited_{dset_name}.json (batch['question_ids'], group tv only: :79-81, :112-114).
    candidates: a decode.AnswerSet or a list of token lists (default: the model's option qa_answer_candidates) -- the same flow with the
    generation constrained to that closed set: every prediction is one of the candidates.
    multiple_choice (default: the model's option qa_multiple_choice): the choices of every question come from
    batch['choice_tokens']['bert_tokens'] (the same count per question inside a batch), the ground truth is the integer index in
    batch['answers'] (or txt_tokens), the prediction is the arg max of decode.score_candidates (the exact sequence log-probability of
    every choice; ties to the lower index); the dumps hold indices. A call that passes neither, on a model without the options, is the
    reference's flow unchanged.
    answer_ranking (default: the model's option qa_answer_ranking, absent = 'decode'): 'decode' -- the constrained generation above;
    'exact' -- with candidates (a shared set): the prediction of every question is the arg max of decode.rank_candidates over the whole
    set (the exact sequence log-probability of every answer; ties to the lower index) instead of what the beam reaches; the rest of the
    flow, the dumps and the accuracy bookkeeping are those of the candidates= mode. 'exact' without candidates, or with
    multiple_choice, raises ValueError."""
    import json
    import os
    from .model.valor import _opt
    from . import decode as D
    core = _unwrapped(model)
    opts = getattr(core, "opts", None)
    multiple_choice = bool(multiple_choice) or bool(_opt(opts, "qa_multiple_choice", False))
    if candidates is None:
        candidates = _opt(opts, "qa_answer_candidates", None)
    if answer_ranking is None:
        answer_ranking = _opt(opts, "qa_answer_ranking", "decode")
    if answer_ranking not in ("decode", "exact"):
        raise ValueError(f"validate_qa: answer_ranking {answer_ranking!r} ('decode' or 'exact')")
    if multiple_choice and candidates is not None:
        raise ValueError("validate_qa: multiple_choice scores the batch's own choices; candidates= (qa_answer_candidates) is the other mode")
    exact = answer_ranking == "exact"
    if exact and multiple_choice:
        raise ValueError("validate_qa: answer_ranking='exact' ranks a shared candidate set; multiple_choice already scores every choice exactly")
    if exact and candidates is None:
        raise ValueError("validate_qa: answer_ranking='exact' needs candidates= (or the option qa_answer_candidates): the set to rank")
    candidates = D._answer_set(candidates)
    if exact and candidates.per_sample:
        raise ValueError("validate_qa: answer_ranking='exact' ranks one shared set; a per-sample set goes through decode.score_candidates")
    if exact:                                   # the answers as '[tokens] [SEP] 0..' rows: what the decoder hands to `dec`
        rows = candidates.candidates[0]
        answer_rows = torch.zeros((len(rows), candidates.max_len + 1), dtype=torch.long)
        for i, r in enumerate(rows):
            answer_rows[i, :len(r)] = torch.tensor(r, dtype=torch.long)
            answer_rows[i, len(r)] = D.EOS
    groups = task.split("%")[1:]
    dec = _decoder(model, decode)
    model.eval()
    gt, submit = [], []
    answers = {g: [] for g in ("tv", "tva", "ta") if g in groups}
    for batch in loader:
        if multiple_choice:
            gt += _answer_indices(batch)
            prompt = core.qa_prompt(batch["question_tokens"]["bert_tokens"].cpu())
            scores = D.score_candidates(core, batch, list(answers), _choice_sets(batch, prompt.shape[0]), prompt_cpu=prompt)
            cols = torch.arange(next(iter(scores.values())).shape[1], device=core.device)
            # the first column that holds the row maximum: ties go to the lower index
            ev = {"generated_answers_" + _GROUP_KEY[g]: torch.where(sc == sc.max(1, keepdim=True).values, cols, cols.numel()).min(1).values.cpu()
                  for g, sc in scores.items()}
            pick = lambda x: [int(i) for i in x]
        elif exact:
            gt += _answer_strings(batch, dec)
            prompt = core.qa_prompt(batch["question_tokens"]["bert_tokens"].cpu())
            top = D.rank_candidates(core, batch, list(answers), candidates, prompt_cpu=prompt, k=1)
            ev = {"generated_answers_" + _GROUP_KEY[g]: answer_rows[idx[:, 0].cpu()] for g, (_, idx) in top.items()}
            pick = dec
        else:
            gt += _answer_strings(batch, dec)
            ev = model(batch, task=task, compute_loss=False, **({} if candidates is None else {"candidates": candidates}))
            pick = dec
        for g in answers:
            a = pick(ev["generated_answers_" + _GROUP_KEY[g]])
            answers[g] += a
            if g == "tv" and batch.get("question_ids") is not None:
                submit += [{"question_id": q, "answer": s} for q, s in zip(batch["question_ids"], a)]
    folder = None
    if output_dir is not None:
        folder = os.path.join(output_dir, "predict_answers")
        os.makedirs(folder, exist_ok=True)

    def dump(obj, name):
        if folder is not None and _rank() == 0:
            with open(os.path.join(folder, name), "w") as fh:
                json.dump(obj, fh)

    gt = _gathered(gt)
    dump(gt, f"step{global_step}_gt.json")
    val_log = {}
    for g in answers:
        pred = _gathered(answers[g])
        if len(pred) != len(gt):
            raise ValueError(f"validate_qa: {len(pred)} answers of group {g} for {len(gt)} ground-truth answers")
        if g == "tv":
            dump(pred, f"step{global_step}_tv_pred.json")
            dump(_gathered(submit), f"step{global_step}_tv_pred_submited_{dset_name}.json")
        acc = sum(p == t for p, t in zip(pred, gt)) / len(gt)
        val_log[g] = {"accuracy": round(acc * 100, 2)}
    return val_log


def validate_single(model, loader, task, *, annotations=None, dset_name="", output_dir=None, global_step=0, **kw):
    """test.py::validate_single (:30-40): route a task string to validate_pt / validate_ret / validate_cap / validate_qa. annotations: the
    caption references of a 'cap' task (default: loader.dataset.annfile, where the reference finds them, test.py:143)."""
    if task.startswith("pt"):
        return validate_pt(model, loader, task)
    if task.startswith("ret"):
        return validate_ret(model, loader, task)
    if task.startswith("cap"):
        if annotations is None:
            annotations = getattr(getattr(loader, "dataset", None), "annfile", None)
        if annotations is None:
            raise ValueError(f"task {task!r}: caption evaluation needs annotations (or loader.dataset.annfile)")
        return validate_cap(model, loader, task, annotations, output_dir=output_dir, global_step=global_step, dset_name=dset_name, **kw)
    if task.startswith("qa"):
        return validate_qa(model, loader, task, decode=kw.get("decode"), output_dir=output_dir, global_step=global_step, dset_name=dset_name,
                           candidates=kw.get("candidates"), multiple_choice=kw.get("multiple_choice", False),
                           answer_ranking=kw.get("answer_ranking"))
    raise NotImplementedError(f"task {task!r}: 'pt', 'ret', 'cap' and 'qa' are the reference's evaluation families (test.py:33-40)")


def validate(model, val_loaders, *, annotations=None, output_dir=None, global_step=0, **kw):
    """test.py::validate (:18-27): val_loaders = {'task--dset': loader}; returns {key: val_log} and puts the model back into train mode.
    annotations: {key or dset name: caption references} for the 'cap' tasks (validate_single's default otherwise)."""
    eval_log = {}
    model.eval()
    try:
        for key, loader in val_loaders.items():
            task, _, dset = key.partition("--")
            ann = None if annotations is None else annotations.get(key, annotations.get(dset))
            eval_log[key] = validate_single(model, loader, task, annotations=ann, dset_name=dset, output_dir=output_dir, global_step=global_step, **kw)
    finally:
        model.train()
    return eval_log
