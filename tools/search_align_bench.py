"""Time the token alignments of search results (RetrievalIndex.explain, search(..., explain=True); csrc/search_align.hip) on synthetic
banks at the 'tva' base geometry (T = 32 text tokens, Nv = 10 clip tokens = 8 video + 2 audio, D = 512), against the only way the
parent commit offers to get such outputs: valor_fine_fused_fwd in its detail mode on the k gathered clips, once per query.

Per bank (bf16; fp8 with a "device" exact store, whose search is the two-stage one), NQ and k, device events around `--iters` warmed calls of
  search            RetrievalIndex.search
  search+explain    search(..., explain=True): the same search, then one valor_fine_align_pairs launch on the returned indices
  explain           RetrievalIndex.explain on the indices of that search alone
  ...+sim           the two above with sim=True (the [NQ, k, T, Nv] similarities written too)
  fused_detail      per query: gather the k clips and their weights, valor_fine_fused_fwd with A2B / B2A / arg-max outputs on [1, k]. It
                    yields the maxima and indices only (no credits, no similarities), so it is a lower bound for the parent commit
the variants alternating inside each of `--rounds` rounds in one process; the median window is reported with the spread. Also the
share of a search that the explanation adds. Writes one JSON document to --out (default profiles/search_align_bench.json) and prints
one line per case. No pass / fail bar: a measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import kernels as K                 # noqa: E402
from valor_amd import lib                          # noqa: E402
from valor_amd import search as S                  # noqa: E402

T, NV, D = 32, 10, 512
LAYOUT = [("video", 8), ("audio", 2)]


def unit_bf16(n, tokens, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n, tokens, D), dtype=torch.bfloat16, device=dev)
    step = 1 << 16
    for i in range(0, n, step):
        m = min(step, n - i)
        out[i:i + m] = torch.nn.functional.normalize(torch.randn((m, tokens, D), generator=g, device=dev), dim=-1).bfloat16()
    return out


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def fused_detail(ft, mask, wq, store, wstore, idx):
    """the parent commit's route: per query, the k clips gathered and valor_fine_fused_fwd in detail mode on [1, k]"""
    NQ, k = idx.shape
    f32, u8 = dict(dtype=torch.float32, device=ft.device), dict(dtype=torch.uint8, device=ft.device)
    ones = torch.ones((k, NV), **f32)
    out = []
    for a in range(NQ):
        rows = idx[a].clamp(min=0)
        fb, wb = store.index_select(0, rows), wstore.index_select(0, rows)
        score, a2b, b2a = torch.empty((1, k), **f32), torch.empty((1, k, T), **f32), torch.empty((1, k, NV), **f32)
        ia, ib = torch.empty((1, k, T), **u8), torch.empty((1, k, NV), **u8)
        lib.call("valor_fine_fused_fwd", K._stream(), ft[a:a + 1].data_ptr(), fb.data_ptr(), mask[a:a + 1].data_ptr(), ones.data_ptr(),
                 wq[a:a + 1].data_ptr(), wb.data_ptr(), score.data_ptr(), a2b.data_ptr(), b2a.data_ptr(), ia.data_ptr(), ib.data_ptr(), 1, k, T, NV, D)
        out.append((score, a2b, b2a, ia, ib))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[10 ** 5])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--k", type=int, nargs="+", default=[10])
    ap.add_argument("--iters", type=int, default=50, help="most calls per timed window (large cases take fewer)")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_align_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "search_align_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    cases = []
    for NB in a.nb:
        g = torch.Generator(device=dev).manual_seed(1)
        fb = unit_bf16(NB, NV, dev, 2)
        wb_raw = torch.randn((NB, NV), generator=g, device=dev)
        bf16 = S.RetrievalIndex.from_features(fb, wb_raw, group="tva", token_layout=LAYOUT)
        banks = {"bf16": bf16, "fp8+device": bf16.quantize(exact="device")}
        for NQ in a.nq:
            fa = unit_bf16(NQ, T, dev, 3)
            wa_raw = torch.randn((NQ, T), generator=g, device=dev)
            mask = (torch.arange(T, device=dev)[None] < torch.randint(8, T + 1, (NQ, 1), generator=g, device=dev)).float()
            q = {"feat_t": fa, "mask": mask, "weight": wa_raw}
            iters = max(3, min(a.iters, int(2e8 / (NB * NQ))))
            for k in a.k:
                for name, index in banks.items():
                    idx = index.search(None, q, k).indices
                    ft, mk, wq = index._queries(None, q)
                    store, wstore = index._pair_store()[0].view(), index.weights[0]
                    variants = {"search": lambda: index.search(None, q, k),
                                "search+explain": lambda: index.search(None, q, k, explain=True),
                                "search+explain+sim": lambda: index.search(None, q, k, explain=True, sim=True),
                                "explain": lambda: index.explain(None, q, idx),
                                "explain+sim": lambda: index.explain(None, q, idx, sim=True),
                                "fused_detail": lambda: fused_detail(ft, mk, wq, store, wstore, idx)}
                    ms = {v: [] for v in variants}
                    for _ in range(a.rounds):
                        for v, fn in variants.items():
                            ms[v].append(timed(fn, iters))
                    med = {v: sorted(x)[len(x) // 2] for v, x in ms.items()}
                    # the two routes agree on what both produce (maxima and indices of the live slots)
                    al, ref = index.explain(None, q, idx).parts[0], fused_detail(ft, mk, wq, store, wstore, idx)
                    same = all(torch.equal(al.text_best[i:i + 1], r[3]) and torch.equal(al.clip_best[i:i + 1], r[4]) and torch.equal(al.text_max[i:i + 1], r[1])
                               and torch.equal(al.clip_max[i:i + 1], r[2]) for i, r in enumerate(ref)) if bool((idx >= 0).all()) else None
                    res = {"bank": name, "NB": NB, "NQ": NQ, "k": k, "iters": iters, "rounds": a.rounds,
                           "ms": {v: round(med[v], 4) for v in variants}, "ms_min_max": {v: [round(min(x), 4), round(max(x), 4)] for v, x in ms.items()},
                           "explain_share_of_search": round(med["explain"] / med["search"], 4),
                           "fused_detail_over_explain": round(med["fused_detail"] / med["explain"], 2),
                           "maxima_and_indices_equal_fused_detail": same}
                    print(json.dumps(res), flush=True)
                    cases.append(res)
        del banks, bf16, fb, wb_raw
        torch.cuda.empty_cache()
    doc = {"bench": "search_align", "geometry": {"T": T, "Nv": NV, "D": D, "token_layout": LAYOUT, "feature_dtype": "bfloat16"},
           "device": torch.cuda.get_device_name(0),
           "timing": "device events over warmed calls; the median of `rounds` windows per variant, the variants alternating inside a round",
           "fused_detail": "valor_fine_fused_fwd with A2B / B2A / arg-max outputs on the k gathered clips, once per query: maxima and indices only",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
