"""Time the caption evaluation metrics at the MSRVTT-test geometry: 2990 clips x 20 references x 5-14 symbols (seeded), one hypothesis
per clip. Prints and writes ONE JSON line:

  device_resident_ms   one DeviceCaptionMetrics.score call with the tables resident: id-matrix upload, both launches, summary readback
                       (host clock around a call that ends in the readback; median and spread over --iters calls after --warmup)
  device_kernels_ms    the two launches alone, between device events (the id matrix already on the device)
  device_cold_s        the first call of a fresh scorer: host statistics, table build, upload, launches
  host_s               capeval.CaptionMetrics.score on the same input, statistics cached (its second call) and cold (its first)

    python tools/capeval_bench.py [--out profiles/capeval_msrvtt_geometry.json]

Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def geometry(seed=0, clips=2990, refs=20, lo=5, hi=14, vocab=8000):
    """words follow a Zipf-like law over `vocab` symbols, so that n-grams repeat across clips as they do in captions"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    word = lambda n: (rng.choice(vocab, size=int(n), p=p) + 1000).tolist()
    corpus = {f"video{i}": [word(rng.integers(lo, hi + 1)) for _ in range(refs)] for i in range(clips)}
    hyps = [list(r[int(rng.integers(refs))][:int(rng.integers(3, 9))]) + word(rng.integers(0, 5)) for r in corpus.values()]
    return corpus, hyps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("capeval_bench: no GPU (a CPU timing says nothing about the device path)")
    from valor_amd import capeval, kernels as K
    dev, eos = "cuda:0", 102
    refs, hyps = geometry()
    ids = list(refs)
    torch.zeros(1, device=dev)                                                 # the context, before any clock starts
    t0 = time.perf_counter()
    dm = capeval.DeviceCaptionMetrics(refs, device=dev, eos=eos)
    first = dm.score(ids, hyps)
    cold = time.perf_counter() - t0
    for _ in range(a.warmup):
        dm.score(ids, hyps)
    calls = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        res = dm.score(ids, hyps)                                              # ends in the summary readback: a synchronising copy
        calls.append((time.perf_counter() - t0) * 1e3)
    assert res.corpus == first.corpus
    # the launches alone
    m, vocab = dm.id_matrix(hyps)
    seq = torch.from_numpy(m).to(dev)
    _, _, _, st, clip_idx = dm._dev
    R = len(ids)
    f64 = torch.empty((6, R), dtype=torch.float64, device=dev)
    counts = torch.empty((R, 10), dtype=torch.int32, device=dev)
    summary = torch.empty(16, dtype=torch.int64, device=dev)
    run = lambda: K.caption_metrics(seq, eos, vocab, clip_idx, st, f64[0], f64[1], f64[2:].view(-1), counts, summary)
    for _ in range(a.warmup):
        run()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for s, e in ev:
        s.record(); run(); e.record()
    torch.cuda.synchronize()
    kern = [s.elapsed_time(e) for s, e in ev]
    t0 = time.perf_counter()
    host = capeval.CaptionMetrics(refs)
    h1 = host.score(ids, hyps)
    host_cold = time.perf_counter() - t0
    t0 = time.perf_counter()
    host.score(ids, hyps)
    host_warm = time.perf_counter() - t0
    worst = max(abs(res.corpus[k] - h1.corpus[k]) / max(abs(h1.corpus[k]), 1e-300) for k in capeval.KEYS)
    q = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    line = dict(bench="capeval", geometry="2990 clips x 20 references x 5-14 symbols, one hypothesis per clip", iters=a.iters,
                device=torch.cuda.get_device_name(0), device_resident_ms=q(calls), device_kernels_ms=q(kern), device_cold_s=round(cold, 3),
                host_s=dict(cold=round(host_cold, 3), statistics_cached=round(host_warm, 3)), table_bytes=int(sum(t.numel() * t.element_size() for t in dm._dev[2].values())),
                corpus={k: round(v * 100, 2) for k, v in res.corpus.items()}, max_rel_diff_device_vs_host=float(worst))
    out = json.dumps(line)
    print(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
