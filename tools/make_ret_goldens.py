"""Fixtures of the retrieval evaluation (tests/golden/ret_metric_*.pt) from the UNMODIFIED reference: its test.compute_metric_ret
(test.py:714-775, with compute_dualsoftmax_forward / _backward :685-712) is imported and called on seeded score matrices; nothing of its
text is copied. Only data is stored: the small matrix whole, the large one as seed + checksum, and for each of the four flag
combinations (dual_softmax x evaluate_ret_text) the reference's eval_log. Beside them, computed here in fp64: the per-query ranks
(stable descending order: ties in index order) and e_ref, the largest relative deviation of the reference's own fp32 dual-softmax
matrices from the same formula in fp64 (over the entries clear of fp32 underflow).

    python tools/make_ret_goldens.py            # needs the reference tree (oracle/ref_harness.py); writes tests/golden/

The helpers below (make_case, fp64_values, stable_ranks, band_counts) are what tests/test_retrieval_*.py import: fixture and test use
one definition of the matrix, of the fp64 rank and of "ambiguous".

Ambiguity. delta = 8 * e_ref of the fixture. A competitor c of a query with ground-truth value t is INSIDE THE BAND if
|c - t| <= max(delta * max(|c|, |t|), floor), where floor = 2^-126 * n * max|score| is the value below which the softmax factor of
score * softmax * n leaves fp32's normal range: no fp32 evaluation of the formula, the reference's included, orders values down there
(a GPU flushes them to zero, the CPU keeps a few denormal bits). A query is ambiguous if any competitor is inside the band; its rank may then lie anywhere between
lo = #{c above the band} and hi = lo + #{c inside the band}. An unambiguous query must have exactly its fp64 rank. (Values that differ
by a relative error e each stay ordered outside a band of 2 e, so the bound leaves an implementation four times the reference's own
deviation. The factor is fixed here and not tuned to any implementation.)
Caps asserted at generation: ambiguous share 0 on the small fixture, <= 5 % on the large one; no exact tie against a ground truth in
the raw matrices (a tie would make the reference's unstable sort the arbiter)."""
import hashlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLAGS = [(False, False), (False, True), (True, False), (True, True)]          # (dual_softmax, evaluate_ret_text)
# name -> (texts per clip, clips, duplicated clip columns, temperature, seed, stored whole)
CASES = {
    "small": dict(per_clip=3, clips=50, dups=((7, 3), (31, 30)), temp=0.07, seed=11, whole=True, max_ambiguous=0.0),
    "large": dict(per_clip=5, clips=2000, dups=(), temp=0.01, seed=5, whole=False, max_ambiguous=0.05),
}
BAND_FACTOR = 8


def make_case(per_clip, clips, dups, seed, **_):
    """(score fp32 [texts, clips], ids, ids_txt): Gaussian scores (std 0.1) with +0.12 on every text's ground-truth column; clip j
    owns the texts j * per_clip ..; `dups` = pairs (column, earlier column) that carry the SAME clip id (ids.index picks the earlier)."""
    g = torch.Generator().manual_seed(seed)
    nt = per_clip * clips
    score = torch.randn((nt, clips), generator=g, dtype=torch.float32) * 0.1
    ids = [f"clip{j}" for j in range(clips)]
    for j, first in dups:
        ids[j] = ids[first]
    ids_txt = [ids[i // per_clip] for i in range(nt)]
    first = {}
    for j, c in enumerate(ids):
        first.setdefault(c, j)
    gt = torch.tensor([first[c] for c in ids_txt])
    score[torch.arange(nt), gt] += 0.12
    perm = torch.randperm(nt, generator=g)                    # texts in loader order, not grouped by clip
    return score[perm].contiguous(), ids, [ids_txt[i] for i in perm.tolist()]


def checksum(score):
    return hashlib.sha1(score.contiguous().numpy().tobytes()).hexdigest()


def gt_columns(ids, ids_txt):
    first = {}
    for j, c in enumerate(ids):
        first.setdefault(c, j)
    return torch.tensor([first[c] for c in ids_txt])


def fp64_values(score, temp, dual):
    """(x, y) fp64: the matrices whose rows / columns are ranked in the forward / backward direction (test.py:694, :710)"""
    s = score.double()
    if not dual:
        return s, s
    z = s / temp
    return s * torch.softmax(z, dim=0) * s.shape[0], s * torch.softmax(z, dim=1) * s.shape[1]


def _count(vals, t, idx_lt, delta, floor=0.0):
    """per query (rows of `vals`; t its threshold, idx_lt marks the candidates with a lower index than the ground truth):
    (stable rank, lo, hi) -- see the module docstring"""
    t = t[:, None]
    rank = ((vals > t) | ((vals == t) & idx_lt)).sum(1)
    band = (delta * torch.maximum(vals.abs(), t.abs())).clamp_min(floor)
    inside = (vals - t).abs() <= band
    lo = ((vals > t) & ~inside).sum(1)
    return rank, lo, lo + inside.sum(1)


def band_counts(score, ids, ids_txt, temp, dual, delta, chunk=1024):
    """fp64 ranks and rank bounds of both directions: dict forward / backward -> (rank, lo, hi) int64 tensors; the ground truth itself
    is excluded from `inside` (hi counts competitors only)."""
    x, y = fp64_values(score, temp, dual)
    nt, nv = x.shape
    gt = gt_columns(ids, ids_txt)
    cols = torch.arange(nv)
    tiny = 2.0 ** -126 * float(score.abs().max()) if dual else 0.0
    out = {"forward": [], "backward": []}
    for a in range(0, nt, chunk):
        xs, g = x[a:a + chunk], gt[a:a + chunk]
        t = xs.gather(1, g[:, None]).squeeze(1)
        r, lo, hi = _count(xs, t, cols[None, :] < g[:, None], delta, tiny * nt)
        out["forward"].append((r, lo, hi - 1))                 # the ground truth is inside its own band
    rows = torch.arange(nt)
    yt = y.t().contiguous()
    for b in range(0, nv, chunk):
        ys = yt[b:b + chunk]                                   # [clips, texts]
        mine = torch.stack([torch.tensor([c == ids[j] for c in ids_txt]) for j in range(b, min(b + chunk, nv))])
        m, istar = ys.masked_fill(~mine, float("-inf")).max(dim=1)
        # the lowest text index that reaches the maximum
        istar = torch.where(mine & (ys == m[:, None]), rows[None, :], torch.full_like(rows, nt)[None, :]).min(dim=1)[0]
        r, lo, hi = _count(ys, m, rows[None, :] < istar[:, None], delta, tiny * nv)
        out["backward"].append((r, lo, hi - 1))
    return {k: tuple(torch.cat([p[i] for p in v]) for i in range(3)) for k, v in out.items()}


def has_exact_tie(score, ids, ids_txt):
    b = band_counts(score, ids, ids_txt, 1.0, False, 0.0)
    return any(bool((hi != lo).any()) for _, lo, hi in b.values())


def host_metrics(rank, prefix):
    """the dict entries of test.py:731-774 from a rank vector (fp32 arithmetic, torch.median = lower middle element)"""
    rank = rank.to(torch.float32)
    n = rank.numel()
    r1, r5, r10 = [(rank < k).sum().item() / n for k in (1, 5, 10)]
    return {f"{prefix}_recall": f"{round(r1 * 100, 1)}/{round(r5 * 100, 1)}/{round(r10 * 100, 1)}", f"{prefix}_ravg": round((r1 + r5 + r10) / 3 * 100, 1),
            f"{prefix}_medianR": torch.median(rank).item() + 1, f"{prefix}_meanR": torch.mean(rank).item() + 1}


# ------------------------------------------------------------------ the reference side (only where its tree is present)
def _reference_test_module():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness
    ref_harness._install()
    for name in ("cococaption", "cococaption.pycocoevalcap", "cococaption.pycocoevalcap.eval", "cococaption.pycocotools", "cococaption.pycocotools.coco"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["cococaption.pycocoevalcap.eval"].COCOEvalCap = None
    sys.modules["cococaption.pycocotools.coco"].COCO = None
    try:
        import tqdm  # noqa: F401
    except ImportError:
        m = types.ModuleType("tqdm")
        m.tqdm = lambda x, *a, **k: x
        sys.modules["tqdm"] = m
    import test as ref_test
    return ref_test


def generate(name):
    ref_test = _reference_test_module()
    cfg = CASES[name]
    score, ids, ids_txt = make_case(**cfg)
    assert not has_exact_tie(score, ids, ids_txt), f"{name}: seed {cfg['seed']} has an exact tie against a ground truth; pick another seed"
    temp = cfg["temp"]
    fix = dict(name=name, per_clip=cfg["per_clip"], clips=cfg["clips"], dups=cfg["dups"], seed=cfg["seed"], temp=temp,
               checksum=checksum(score), eval_log={}, ranks={})
    if cfg["whole"]:
        fix.update(score=score, ids=ids, ids_txt=ids_txt)
    e_ref = 0.0
    for dual, text in FLAGS:
        model = types.SimpleNamespace(video_encoder_type="videoswin", contra_temp=temp, dual_softmax=dual, evaluate_ret_text=text)
        with torch.no_grad():
            fix["eval_log"][(dual, text)] = ref_test.compute_metric_ret(score.clone(), list(ids), list(ids_txt), model)
            if dual and text:
                x32 = ref_test.compute_dualsoftmax_forward(score.clone(), model, ids_txt)[0]
                y32 = ref_test.compute_dualsoftmax_backward(score.clone(), model)
                for v32, v64 in zip((x32, y32), fp64_values(score, temp, True)):
                    ok = v64.abs() >= 1e-30                     # clear of fp32 underflow, where a relative deviation means nothing
                    e_ref = max(e_ref, float(((v32.double() - v64).abs()[ok] / v64.abs()[ok]).max()))
    fix["e_ref"] = e_ref
    for dual in (False, True):
        b = band_counts(score, ids, ids_txt, temp, dual, BAND_FACTOR * e_ref if dual else 0.0)
        fix["ranks"][dual] = {k: v[0].to(torch.int32) for k, v in b.items()}
        if dual:
            amb = {k: float((v[1] != v[2]).double().mean()) for k, v in b.items()}
            fix["ambiguous_share"] = amb
            assert max(amb.values()) <= cfg["max_ambiguous"], (name, amb)
        # the reference's own log from its own (fp32, unstable-sort) ranks against the fp64 stable ranks: equal without dual softmax
        if not dual:
            want = dict(host_metrics(fix["ranks"][False]["forward"], "forward"), **host_metrics(fix["ranks"][False]["backward"], "backward"))
            assert fix["eval_log"][(False, True)] == want, (fix["eval_log"][(False, True)], want)
    return fix


def main():
    for name in CASES:
        fix = generate(name)
        path = os.path.join(GOLDEN, f"ret_metric_{name}.pt")
        torch.save(fix, path)
        print(name, "e_ref", fix["e_ref"], "ambiguous", fix.get("ambiguous_share"), os.path.getsize(path), "bytes")
        for k, v in fix["eval_log"].items():
            print("  ", k, v)


if __name__ == "__main__":
    main()
