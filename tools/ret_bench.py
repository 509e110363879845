"""Time the retrieval ranking at MSCOCO size (25000 captions x 5000 images, a seeded fp32 matrix already on the device).

    python tools/ret_bench.py forward [--out FILE]    retrieval_metrics, text -> clip only, no dual softmax, against compute_metric_ret (the
                                                      sort + tolist + list.index of the parent) on the same matrix: the like-for-like pair
    python tools/ret_bench.py dual [--out FILE]       both directions with dual softmax (no counterpart in the parent)
    python tools/ret_bench.py trace                   a few calls of each, for a kernel trace by an external profiler

Each mode is one process; run each under its own time limit. Prints one JSON line with the times and the HBM floor: matrix bytes x
passes / 6.3e12 B/s (what a device copy reaches)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NT, NV, PER = 25000, 5000, 5
HBM = 6.3e12


def _case(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    score = torch.randn((NT, NV), generator=g, device=dev) * 0.2
    ids = [f"c{j}" for j in range(NV)]
    ids_txt = [ids[i // PER] for i in range(NT)]
    score[torch.arange(NT, device=dev), torch.arange(NT, device=dev) // PER] += 0.12
    return score, ids, ids_txt


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return sorted(ts)[len(ts) // 2], min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["forward", "dual", "trace"])
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from valor_amd.evaluate import _gt_columns, compute_metric_ret, retrieval_metrics, retrieval_ranks
    dev = torch.device("cuda:0")
    score, ids, ids_txt = _case(dev)
    mb = NT * NV * 4
    res = dict(mode=a.mode, texts=NT, clips=NV, matrix_bytes=mb)
    if a.mode == "forward":
        med, best = _time(lambda: retrieval_metrics(score, ids, ids_txt), a.reps)
        gt = _gt_columns(ids, ids_txt, False)[0]
        gt_dev = torch.tensor(gt, dtype=torch.int32, device=dev)
        kmed, kbest = _time(lambda: retrieval_ranks(score, gt_dev), a.reps)
        new = retrieval_metrics(score, ids, ids_txt)
        t = time.perf_counter()
        old = compute_metric_ret(score.cpu(), ids, ids_txt)              # what validate_pt does: the matrix to the host, sort, tolist, index
        t_old = time.perf_counter() - t
        res.update(retrieval_metrics_s=med, retrieval_metrics_best_s=best, ranks_only_s=kmed, parent_compute_metric_ret_s=t_old,
                   same_log=(new == old), passes=1, hbm_floor_s=mb / HBM)
    elif a.mode == "dual":
        med, best = _time(lambda: retrieval_metrics(score, ids, ids_txt, dual_softmax=True, temp=0.01, text_direction=True), a.reps)
        gt, ptr, rows = _gt_columns(ids, ids_txt, True)
        to = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
        gt, ptr, rows = to(gt), to(ptr), to(rows)
        kmed, kbest = _time(lambda: retrieval_ranks(score, gt, ptr, rows, dual_softmax=True, temp=0.01), a.reps)
        res.update(retrieval_metrics_s=med, retrieval_metrics_best_s=best, ranks_only_s=kmed, passes=2, hbm_floor_s=2 * mb / HBM)
    else:
        gt, ptr, rows = _gt_columns(ids, ids_txt, True)
        to = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
        gt, ptr, rows = to(gt), to(ptr), to(rows)
        for _ in range(3):
            retrieval_ranks(score, gt)
            retrieval_ranks(score, gt, ptr, rows, dual_softmax=True, temp=0.01)
        torch.cuda.synchronize()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
