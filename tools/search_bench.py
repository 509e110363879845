"""Time RetrievalIndex.search on synthetic bf16 banks at the pretraining token geometry (T = 32 text tokens, Nv = 10 clip tokens, D = 512)
against what the parent commit offers for the same question: evaluate.fine_score_matrix over the whole bank followed by torch.topk.

Per (NB, NQ, k): device events around `--iters` warmed calls of
  search     RetrievalIndex.search (chunked fused scoring + valor_topk_rows per chunk)
  topk       the valor_topk_rows calls of that search alone, on a score buffer of the chunk's shape: its share of the search
  baseline   fine_score_matrix(whole bank) + torch.topk, wherever the [NQ, NB] fp32 matrix fits beside the bank
and the rate at which the search reads the bank (features + token weights, the bytes the algorithm must read once per query batch) against
the HBM rates of the MI355X (8.0 TB/s peak, about 6.3 TB/s achievable). The score path is compute-bound for many queries (NQ * T * Nv * D
multiply-adds per clip), so the bank rate is an end-to-end figure of the search, not a kernel's share of peak.
Also reports valor_topk_rows alone on [NQ, NB] fp32 scores (4 bytes per pair): the kernel's own bound is that read.

Writes one JSON document to --out (default profiles/search_bench.json) and prints one line per case. No pass / fail bar: a measurement.

--bank-dtype fp8 | both (default bf16: the run above, unchanged) times the fp8 bank (RetrievalIndex bank_dtype="fp8": e4m3 codes + row
scales, valor_fine_fused_fwd_fp8) instead of / beside the bf16 bank, on the same shapes, features and queries in one process: `--rounds`
timed windows per bank, alternating bf16, fp8, bf16, ... so that drift of the shared host hits both alike; the median window is reported
with the spread. Per (NB, NQ, k): search ms, bank bytes (RetrievalIndex.bank_bytes) and bank read GB/s of each bank, the ratio, and the
share of the bf16 bank's top-k clips that the fp8 bank returns too (the banks are random unit vectors: neighbouring scores lie closer
than the quantisation error, so this is a lower bound for structured data). Default --out profiles/search_fp8_bench.json.

--rescore times the two-stage search (an fp8 bank with an exact store: the fp8 walk returns a shortlist, valor_fine_score_pairs re-scores
it on the bf16 features, the exact top k is returned) on the same shapes, in one process, the variants alternating inside each of
`--rounds` rounds: the bf16 bank (exhaustive, the answer the others are held to), the fp8 bank alone (shortlist=0), and the fp8 bank with
a "device" and with a "host" store at shortlists of k, 2 k, 4 k and 256. Per (NB, NQ, k) and variant: the median ms per search with the
spread, the time over the fp8-only search of the same run, and the share of the bf16 bank's k best clips that the variant returns.
The host store's search synchronises once per call (device events still span it: the stream idles meanwhile). Default --out
profiles/search_rescore_bench.json.

--bank-dtype mxfp4 | all times the MXFP4 bank (RetrievalIndex bank_dtype="mxfp4": MX e2m1 codes + E8M0 block scale bytes, queries
quantised per call to MX e4m3, valor_fine_fused_fwd_mx on the block-scaled MFMA) alone / beside the bf16 and the fp8 bank, on the same
shapes, features and queries in one process, in alternating timed windows as above (bf16, fp8, mxfp4, bf16, ...). Per (NB, NQ, k) and
bank: the median search ms with the spread, the bank bytes and read rate, the time over the fp8 bank of the same run, and the share of
the bf16 bank's top-k clips that the code bank alone returns. With --rescore the mxfp4 bank also keeps a "device" store and the
two-stage search is timed at shortlists of k, 4 k, 8 k and 256, with the share of the bf16 top k it returns (the exact answer wherever
the shortlist holds it). Default --out profiles/search_mx_bench.json.

--removed-frac F and / or --group-size G time the selection with removal, a filter and one result per group (valor_topk_rows_select) on
the bf16 bank, beside the plain search of the same bank (valor_topk_rows: the walk an index that removed nothing runs, unchanged), the
variants alternating inside each of `--rounds` rounds: "plain"; "removed" (a share F of the clips tombstoned at random); "where" (a
filter admitting a share 1 - F, nothing removed); "collapse" (consecutive groups of G clips, one result per group); "removed+collapse".
Per (NB, NQ, k) and variant: the median ms per search with the spread and the time over the plain search. The selection calls alone
(valor_topk_rows / valor_topk_rows_select over the chunks of one walk, on a score buffer of the chunk's shape) are timed the same way.
--parent FILE adds the plain search of another build to the document: FILE is what the default mode of this tool (no --bank-dtype, no
--rescore) wrote when run from the parent commit's tree on the same machine; its search_ms and topk_ms are kept per (NB, NQ, k) under
"parent_plain_search". Default --out profiles/search_select_bench.json."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import evaluate as E                # noqa: E402
from valor_amd import search as S                  # noqa: E402

T, NV, D = 32, 10, 512
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


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


def compare_banks(a, dev):
    """--bank-dtype fp8 / both"""
    kinds = ("bf16", "fp8") if a.bank_dtype == "both" else ("fp8",)
    free = torch.cuda.mem_get_info()[0]
    cases = []
    for NB in a.nb:
        if NB * NV * (D * 3 + 12) * 1.2 > free:
            print(f"NB={NB}: the two banks do not fit", flush=True)
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        fb = unit_bf16(NB, NV, dev, 2)
        wb_raw = torch.randn((NB, NV), generator=g, device=dev)
        banks = {"bf16": S.RetrievalIndex.from_features(fb, wb_raw, group="tva")}
        banks["fp8"] = banks["bf16"].quantize()
        if "bf16" not in kinds:
            del banks["bf16"], fb
        for NQ in a.nq:
            fa = unit_bf16(NQ, T, dev, 3)
            wa_raw = torch.randn((NQ, T), generator=g, device=dev)
            mask = (torch.arange(T, device=dev)[None] < torch.randint(8, T + 1, (NQ, 1), generator=g, device=dev)).float()
            q = {"feat_t": fa, "mask": mask, "weight": wa_raw}
            iters = max(3, min(a.iters, int(2e8 / (NB * NQ))))
            for k in a.k:
                ms = {kind: [] for kind in kinds}
                for _ in range(a.rounds):
                    for kind in kinds:
                        ms[kind].append(timed(lambda: banks[kind].search(None, q, k), iters))
                res = {"NB": NB, "NQ": NQ, "k": k, "iters": iters, "rounds": a.rounds}
                for kind in kinds:
                    med = sorted(ms[kind])[len(ms[kind]) // 2]
                    nbytes = banks[kind].bank_bytes()
                    res.update({f"{kind}_search_ms": round(med, 4), f"{kind}_search_ms_min_max": [round(min(ms[kind]), 4), round(max(ms[kind]), 4)],
                                f"{kind}_chunk": banks[kind].default_chunk(NQ, T), f"{kind}_bank_GB": round(nbytes / 1e9, 4),
                                f"{kind}_bank_GBps": round(nbytes / med / 1e6, 1)})
                if len(kinds) == 2:
                    res["bf16_over_fp8"] = round(res["bf16_search_ms"] / res["fp8_search_ms"], 3)
                    got, want = banks["fp8"].search(None, q, k).indices.cpu().tolist(), banks["bf16"].search(None, q, k).indices.cpu().tolist()
                    res["topk_overlap"] = round(sum(len(set(g_) & set(w_)) for g_, w_ in zip(got, want)) / (min(k, NB) * NQ), 4)
                    diff = (banks["fp8"].scores(None, q) - banks["bf16"].scores(None, q)).abs().max() if NB * NQ * 4 * 4 < free else None
                    res["largest_score_difference"] = None if diff is None else round(float(diff), 6)
                print(json.dumps(res), flush=True)
                cases.append(res)
        banks.clear()
        fb = wb_raw = None
        torch.cuda.empty_cache()
    return {"bench": "search_fp8", "geometry": {"T": T, "Nv": NV, "D": D, "feature_dtype": "bfloat16", "banks": list(kinds)},
            "device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12, "hbm_achievable_TBps": HBM_ACHIEVABLE / 1e12,
            "timing": "device events over warmed calls; the median of `rounds` windows per bank, the banks alternating", "cases": cases}


def compare_rescore(a, dev):
    """--rescore"""
    free = torch.cuda.mem_get_info()[0]
    cases = []
    for NB in a.nb:
        if NB * NV * (D * 6 + 24) * 1.2 > free:                         # bf16 bank, two code banks, the device store
            print(f"NB={NB}: the banks do not fit", flush=True)
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        fb = unit_bf16(NB, NV, dev, 2)
        wb_raw = torch.randn((NB, NV), generator=g, device=dev)
        bf16 = S.RetrievalIndex.from_features(fb, wb_raw, group="tva")
        on_dev, on_host = bf16.quantize(exact="device"), bf16.quantize(exact="host")
        for NQ in a.nq:
            fa = unit_bf16(NQ, T, dev, 3)
            wa_raw = torch.randn((NQ, T), generator=g, device=dev)
            mask = (torch.arange(T, device=dev)[None] < torch.randint(8, T + 1, (NQ, 1), generator=g, device=dev)).float()
            q = {"feat_t": fa, "mask": mask, "weight": wa_raw}
            iters = max(3, min(a.iters, int(2e8 / (NB * NQ))))
            for k in a.k:
                shortlists = sorted({min(s_, S.MAX_SHORTLIST) for s_ in (k, 2 * k, 4 * k, S.MAX_SHORTLIST)})
                variants = {"bf16": lambda: bf16.search(None, q, k), "fp8": lambda: on_dev.search(None, q, k, shortlist=0)}
                for s_ in shortlists:
                    variants[f"fp8+device/{s_}"] = lambda s_=s_: on_dev.search(None, q, k, shortlist=s_)
                    variants[f"fp8+host/{s_}"] = lambda s_=s_: on_host.search(None, q, k, shortlist=s_)
                ms = {name: [] for name in variants}
                for _ in range(a.rounds):
                    for name, fn in variants.items():
                        ms[name].append(timed(fn, iters))
                want = variants["bf16"]().indices.cpu().tolist()
                med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
                res = {"NB": NB, "NQ": NQ, "k": k, "iters": iters, "rounds": a.rounds, "default_shortlist": on_dev.default_shortlist(k), "variants": {}}
                for name, fn in variants.items():
                    got = fn().indices.cpu().tolist()
                    res["variants"][name] = {
                        "search_ms": round(med[name], 4), "search_ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                        "over_fp8_only": round(med[name] / med["fp8"], 3),
                        "topk_overlap": round(sum(len(set(g_) & set(w_)) for g_, w_ in zip(got, want)) / (min(k, NB) * NQ), 4)}
                res["device_bytes_GB"] = {"bf16": round(bf16.bank_bytes() / 1e9, 4), "fp8+device": round(on_dev.bank_bytes() / 1e9, 4),
                                          "fp8+host": round(on_host.bank_bytes() / 1e9, 4)}
                print(json.dumps(res), flush=True)
                cases.append(res)
        del bf16, on_dev, on_host, fb, wb_raw
        torch.cuda.empty_cache()
    return {"bench": "search_rescore", "geometry": {"T": T, "Nv": NV, "D": D, "feature_dtype": "bfloat16"}, "device": torch.cuda.get_device_name(0),
            "timing": "device events over warmed calls; the median of `rounds` windows per variant, the variants alternating inside a round",
            "overlap": "share of the bf16 bank's k best clips that the variant returns (random unit vectors: a lower bound for structured data)",
            "cases": cases}


def compare_mx(a, dev):
    """--bank-dtype mxfp4 / all (with or without --rescore)"""
    kinds = ("bf16", "fp8", "mxfp4") if a.bank_dtype == "all" else ("mxfp4",)
    free = torch.cuda.mem_get_info()[0]
    cases = []
    overlap = lambda got, want, k, NB, NQ: round(sum(len(set(g_) & set(w_)) for g_, w_ in zip(got, want)) / (min(k, NB) * NQ), 4)
    for NB in a.nb:
        if NB * NV * (D * (5.6 if a.rescore else 3.6) + 24) * 1.2 > free:         # bf16 bank, fp8 and mxfp4 codes, the device store
            print(f"NB={NB}: the banks do not fit", flush=True)
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        fb = unit_bf16(NB, NV, dev, 2)
        wb_raw = torch.randn((NB, NV), generator=g, device=dev)
        bf16 = S.RetrievalIndex.from_features(fb, wb_raw, group="tva")
        banks = {"bf16": bf16, "fp8": bf16.quantize(), "mxfp4": bf16.quantize(bank_dtype="mxfp4")}
        banks = {kind: banks[kind] for kind in kinds}
        stored = bf16.quantize(bank_dtype="mxfp4", exact="device") if a.rescore else None
        for NQ in a.nq:
            fa = unit_bf16(NQ, T, dev, 3)
            wa_raw = torch.randn((NQ, T), generator=g, device=dev)
            mask = (torch.arange(T, device=dev)[None] < torch.randint(8, T + 1, (NQ, 1), generator=g, device=dev)).float()
            q = {"feat_t": fa, "mask": mask, "weight": wa_raw}
            iters = max(3, min(a.iters, int(2e8 / (NB * NQ))))
            for k in a.k:
                variants = {kind: (lambda kind=kind: banks[kind].search(None, q, k)) for kind in kinds}
                if stored is not None:
                    for s_ in sorted({min(s_, S.MAX_SHORTLIST) for s_ in (k, 4 * k, 8 * k, S.MAX_SHORTLIST)}):
                        variants[f"mxfp4+device/{s_}"] = lambda s_=s_: stored.search(None, q, k, shortlist=s_)
                ms = {name: [] for name in variants}
                for _ in range(a.rounds):
                    for name, fn in variants.items():
                        ms[name].append(timed(fn, iters))
                med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
                want = bf16.search(None, q, k).indices.cpu().tolist()
                res = {"NB": NB, "NQ": NQ, "k": k, "iters": iters, "rounds": a.rounds, "variants": {}}
                if stored is not None:
                    res["default_shortlist"] = stored.default_shortlist(k)
                for name, fn in variants.items():
                    row = {"search_ms": round(med[name], 4), "search_ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                           "topk_overlap_with_bf16": overlap(fn().indices.cpu().tolist(), want, k, NB, NQ)}
                    if name in banks:
                        nbytes = banks[name].bank_bytes()
                        row.update(chunk=banks[name].default_chunk(NQ, T), bank_GB=round(nbytes / 1e9, 4), bank_GBps=round(nbytes / med[name] / 1e6, 1))
                    if "fp8" in med:
                        row["over_fp8"] = round(med[name] / med["fp8"], 3)
                    if name != "mxfp4":
                        row["over_mxfp4_only"] = round(med[name] / med["mxfp4"], 3)
                    res["variants"][name] = row
                if stored is not None:
                    res["mxfp4+device_bank_GB"] = round(stored.bank_bytes() / 1e9, 4)
                if NB * NQ * 4 * 4 < free:
                    res["largest_score_difference_mxfp4_bf16"] = round(float((banks["mxfp4"].scores(None, q) - bf16.scores(None, q)).abs().max()), 6)
                print(json.dumps(res), flush=True)
                cases.append(res)
        banks.clear()
        del bf16, stored, fb, wb_raw
        torch.cuda.empty_cache()
    return {"bench": "search_mx", "geometry": {"T": T, "Nv": NV, "D": D, "feature_dtype": "bfloat16", "banks": list(kinds), "rescore": bool(a.rescore)},
            "device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12, "hbm_achievable_TBps": HBM_ACHIEVABLE / 1e12,
            "timing": "device events over warmed calls; the median of `rounds` windows per variant, the variants alternating inside a round",
            "overlap": "share of the bf16 bank's k best clips that the variant returns (random unit vectors: a lower bound for structured data)",
            "cases": cases}


def compare_select(a, dev):
    """--removed-frac / --group-size"""
    free = torch.cuda.mem_get_info()[0]
    frac, gsize = a.removed_frac or 0.0, a.group_size or 0
    cases = []
    for NB in a.nb:
        if NB * NV * (D * 2 + 4) * 1.2 > free:
            print(f"NB={NB}: the bank does not fit", flush=True)
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        fb = unit_bf16(NB, NV, dev, 2)
        wb_raw = torch.randn((NB, NV), generator=g, device=dev)
        labels = [j // gsize for j in range(NB)] if gsize else None
        make = lambda groups=None: S.RetrievalIndex.from_features(fb, wb_raw, group="tva", groups=groups)      # the banks alias fb
        plain = make()
        gone = torch.nonzero(torch.rand(NB, generator=g, device=dev) < frac).view(-1)
        where = torch.rand(NB, generator=g, device=dev) >= frac
        variants = {"plain": (plain, {})}
        if frac:
            removed = make()
            removed.remove(indices=gone)
            variants.update({"removed": (removed, {}), "where": (plain, {"where": where})})
        if gsize:
            grouped = make(labels)
            variants["collapse"] = (grouped, {"collapse": True})
            if frac:
                both = make(labels)
                both.remove(indices=gone)
                variants["removed+collapse"] = (both, {"collapse": True})
        for NQ in a.nq:
            fa = unit_bf16(NQ, T, dev, 3)
            wa_raw = torch.randn((NQ, T), generator=g, device=dev)
            mask = (torch.arange(T, device=dev)[None] < torch.randint(8, T + 1, (NQ, 1), generator=g, device=dev)).float()
            q = {"feat_t": fa, "mask": mask, "weight": wa_raw}
            chunk = plain.default_chunk(NQ, T)
            iters = max(3, min(a.iters, int(2e8 / (NB * NQ))))
            bufs = [torch.randn((NQ, min(chunk, NB)), device=dev)]
            for k in a.k:
                state = (torch.full((NQ, k), float("-inf"), device=dev), torch.full((NQ, k), -1, dtype=torch.int64, device=dev))
                ws = torch.empty((max(S.topk_select_workspace_bytes(NQ, b.shape[1], k) for b in bufs),), dtype=torch.uint8, device=dev)

                def selection(index, kw):
                    keep, group = index._selection(kw.get("where"), kw.get("collapse", False), NQ)
                    for c0 in range(0, NB, chunk):
                        b = bufs[0][:, :min(chunk, NB - c0)]
                        if keep is None and group is None:
                            S.topk_rows(b, k, col_base=c0, state=state, workspace=ws)
                        else:
                            S.topk_rows_select(b, k, col_base=c0, state=state, workspace=ws, keep=keep, group=group, check_state=False)   # as the index calls it

                fns = {name: (lambda index=index, kw=kw: index.search(None, q, k, **kw)) for name, (index, kw) in variants.items()}
                sel = {name: (lambda index=index, kw=kw: selection(index, kw)) for name, (index, kw) in variants.items()}
                ms, sel_ms = {name: [] for name in fns}, {name: [] for name in fns}
                for _ in range(a.rounds):
                    for name in fns:
                        ms[name].append(timed(fns[name], iters))
                        sel_ms[name].append(timed(sel[name], iters))
                med = lambda v: sorted(v)[len(v) // 2]
                res = {"NB": NB, "NQ": NQ, "k": k, "chunk": chunk, "iters": iters, "rounds": a.rounds, "variants": {}}
                for name in fns:
                    res["variants"][name] = {"search_ms": round(med(ms[name]), 4), "search_ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                                             "over_plain": round(med(ms[name]) / med(ms["plain"]), 3), "selection_ms": round(med(sel_ms[name]), 4),
                                             "selection_over_plain": round(med(sel_ms[name]) / med(sel_ms["plain"]), 3),
                                             "results": int((fns[name]().indices >= 0).sum()) // NQ}
                print(json.dumps(res), flush=True)
                cases.append(res)
        variants.clear()
        del plain, fb, wb_raw
        torch.cuda.empty_cache()
    parent = None
    if a.parent:
        with open(a.parent) as fh:
            theirs = json.load(fh)
        parent = {"what": "the default mode of tools/search_bench.py run from the parent commit's tree on the same machine (--parent): the plain "
                          "search and its valor_topk_rows calls alone",
                  "cases": [{key: c[key] for key in ("NB", "NQ", "k", "search_ms", "topk_ms")} for c in theirs["cases"]]}
    return {"bench": "search_select", "parent_plain_search": parent, "geometry": {"T": T, "Nv": NV, "D": D, "feature_dtype": "bfloat16"}, "device": torch.cuda.get_device_name(0),
            "removed_frac": frac, "group_size": gsize,
            "timing": "device events over warmed calls; the median of `rounds` windows per variant, the variants alternating inside a round",
            "plain": "an index that removed nothing, has no groups and gets no filter: valor_topk_rows, the walk of the parent commit",
            "selection_ms": "the selection calls of one walk alone, on random scores of the chunk's shape", "cases": cases}


def write(doc, out):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[10 ** 4, 10 ** 5, 10 ** 6])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--iters", type=int, default=200, help="most calls per timed window (large cases take fewer)")
    ap.add_argument("--bank-dtype", choices=("bf16", "fp8", "both", "mxfp4", "all"), default="bf16",
                    help="fp8 / both: the fp8 bank instead of / beside the bf16 bank; mxfp4 / all: the MXFP4 bank alone / beside the bf16 and the fp8 bank")
    ap.add_argument("--rounds", type=int, default=3, help="--bank-dtype fp8 / both: timed windows per bank")
    ap.add_argument("--rescore", action="store_true", help="the two-stage search on an fp8 bank with an exact store beside the bf16 and the fp8-only search")
    ap.add_argument("--removed-frac", type=float, default=None, help="the selection with this share of the clips removed / filtered out, beside the plain search")
    ap.add_argument("--parent", default=None, help="with --removed-frac / --group-size: the search_bench.json the parent commit's tool wrote on this machine")
    ap.add_argument("--group-size", type=int, default=None, help="the selection with one result per group of this many consecutive clips, beside the plain search")
    ap.add_argument("--out", default=None, help="default profiles/search_bench.json (bf16), profiles/search_fp8_bench.json (fp8, both) or "
                                                "profiles/search_rescore_bench.json (--rescore); profiles/search_mx_bench.json (mxfp4, all)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "search_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    if a.removed_frac is not None or a.group_size is not None:
        if not 0.0 <= (a.removed_frac or 0.0) < 1.0 or (a.group_size or 1) < 1 or a.bank_dtype != "bf16" or a.rescore:
            ap.error("--removed-frac in [0, 1), --group-size >= 1, on the bf16 bank")
        write(compare_select(a, dev), a.out or os.path.join(ROOT, "profiles", "search_select_bench.json"))
        return
    if a.bank_dtype in ("mxfp4", "all"):
        write(compare_mx(a, dev), a.out or os.path.join(ROOT, "profiles", "search_mx_bench.json"))
        return
    if a.rescore:
        write(compare_rescore(a, dev), a.out or os.path.join(ROOT, "profiles", "search_rescore_bench.json"))
        return
    if a.bank_dtype != "bf16":
        write(compare_banks(a, dev), a.out or os.path.join(ROOT, "profiles", "search_fp8_bench.json"))
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "search_bench.json")
    free = torch.cuda.mem_get_info()[0]
    cases = []
    for NB in a.nb:
        bank_bytes = NB * NV * (D * 2 + 4)
        if bank_bytes * 1.2 > free:
            print(f"NB={NB}: a bank of {bank_bytes / 1e9:.1f} GB does not fit", flush=True)
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        fb = unit_bf16(NB, NV, dev, 2)
        wb_raw = torch.randn((NB, NV), generator=g, device=dev)
        index = S.RetrievalIndex.from_features(fb, wb_raw, group="tva")
        ones_b = torch.ones((NB, NV), device=dev)
        for NQ in a.nq:
            fa = unit_bf16(NQ, T, dev, 3)
            wa_raw = torch.randn((NQ, T), generator=g, device=dev)
            mask = (torch.arange(T, device=dev)[None] < torch.randint(8, T + 1, (NQ, 1), generator=g, device=dev)).float()
            q = {"feat_t": fa, "mask": mask, "weight": wa_raw}
            chunk = index.default_chunk(NQ, T)
            iters = max(3, min(a.iters, int(2e8 / (NB * NQ))))                        # about the same work per timed window
            full = index.scores(None, q) if NB * NQ * 4 * 3 < free else None
            for k in a.k:
                search_ms = timed(lambda: index.search(None, q, k), iters)
                bufs = [torch.randn((NQ, min(chunk, NB - c0)), device=dev) for c0 in range(0, NB, chunk)][:2]
                state = (torch.full((NQ, k), float("-inf"), device=dev), torch.full((NQ, k), -1, dtype=torch.int64, device=dev))
                ws = torch.empty((max(S.topk_workspace_bytes(NQ, b.shape[1], k) for b in bufs),), dtype=torch.uint8, device=dev)

                def topk_only():
                    for c0 in range(0, NB, chunk):
                        b = bufs[0] if NB - c0 >= chunk else bufs[-1]
                        S.topk_rows(b, k, col_base=c0, state=state, workspace=ws)

                topk_ms = timed(topk_only, iters)
                res = {"NB": NB, "NQ": NQ, "k": k, "chunk": chunk, "iters": iters, "search_ms": round(search_ms, 4), "topk_ms": round(topk_ms, 4),
                       "topk_share": round(topk_ms / search_ms, 4), "bank_GB": round(bank_bytes / 1e9, 3),
                       "bank_GBps": round(bank_bytes / search_ms / 1e6, 1), "bank_rate_of_hbm_peak": round(bank_bytes / (search_ms * 1e-3) / HBM_PEAK, 4),
                       "bank_rate_of_hbm_achievable": round(bank_bytes / (search_ms * 1e-3) / HBM_ACHIEVABLE, 4),
                       "score_GFLOPs": round(2.0 * NQ * T * NB * NV * D / 1e9, 2),
                       "score_TFLOPps": round(2.0 * NQ * T * NB * NV * D / (search_ms * 1e-3) / 1e12, 2)}
                if full is not None:
                    def baseline():
                        m = E.fine_score_matrix(fa, fb, mask, ones_b, wa_raw, wb_raw)
                        return torch.topk(m, min(k, NB), dim=1)

                    res["baseline_ms"] = round(timed(baseline, iters), 4)
                    res["baseline_over_search"] = round(res["baseline_ms"] / search_ms, 3)
                    topk_full_ms = timed(lambda: S.topk_rows(full, k), iters)
                    torch_topk_ms = timed(lambda: torch.topk(full, min(k, NB), dim=1), iters)
                    res.update(topk_rows_full_matrix_ms=round(topk_full_ms, 4), torch_topk_full_matrix_ms=round(torch_topk_ms, 4),
                               topk_rows_full_matrix_GBps=round(NQ * NB * 4 / topk_full_ms / 1e6, 1))
                    # the two agree wherever the k-th and (k+1)-th scores differ (torch.topk leaves the order of equal values open)
                    got = index.search(None, q, k)
                    want = torch.topk(full, min(k, NB), dim=1)
                    res["indices_equal_torch_topk"] = bool(torch.equal(got.indices[:, :min(k, NB)], want.indices))
                else:
                    res["baseline_ms"] = None
                print(json.dumps(res), flush=True)
                cases.append(res)
        del index, fb, wb_raw, ones_b
        torch.cuda.empty_cache()
    doc = {"bench": "search", "geometry": {"T": T, "Nv": NV, "D": D, "dtype": "bfloat16"}, "device": torch.cuda.get_device_name(0),
           "hbm_peak_TBps": HBM_PEAK / 1e12, "hbm_achievable_TBps": HBM_ACHIEVABLE / 1e12, "timing": "device events over warmed calls", "cases": cases}
    write(doc, a.out)


if __name__ == "__main__":
    main()
