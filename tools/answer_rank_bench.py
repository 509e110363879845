"""Exact ranking of a whole closed answer set: decode.rank_candidates (level-batched trie scoring, one decoder row per trie node)
against decode.score_candidates (forced decoding, one row per candidate and step), on the bench model (VALOR-base widths) at 64 clips of
8 frames + 2 audio slices, one question per clip, group 'tva', V = 30522, for synthetic shared sets of 1500 and 3129 answers of 1..4
tokens with common prefixes (synth.make_answer_set), in fp32 and bf16.
  * both paths alternate in ONE process after a warm-up call of each; a figure is the median of its runs, every run ends in a device
    synchronise and includes the encoders (both paths run them once per call);
  * the decoder rows each path ran are counted from the sets (score_candidates pads its last chunk: the padded rows are counted),
    the peak memory is torch's allocator peak over the path's runs, and the two results are compared (max |difference| of a score);
  * one valor_trie_score_level launch on 8192 rows of the padded logits of the 3129-answer set, between device events, with the
    log-sum-exp computed in the launch and handed in, for two shapes: every row on the root (b = 8192: each row scores the root's
    children, the edge stores at their most) and a chunk as the pass issues it (128 nodes of level 1 x 64 samples); the row bytes
    over the time of the first variant is the achieved stream rate.
The result file is rewritten after every cell (a cell = one dtype x one set; it records its own runs); --resume reads an existing result
file and measures only the cells it lacks, so a long measurement can be taken in several calls. Progress goes to stderr.
usage: python tools/answer_rank_bench.py [out.json] [batch] [rounds] [--plan] [--resume]
       (default profiles/answer_rank_bench.json 64 3; --plan prints the sets' row counts and needs no device)"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from valor_amd import decode, kernels as K, synth  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAN, RESUME = "--plan" in sys.argv, "--resume" in sys.argv
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "answer_rank_bench.json")
B = int(ARGS[1]) if len(ARGS) > 1 else 64
ROUNDS = int(ARGS[2]) if len(ARGS) > 2 else 3
V = 30522
SCORE_ROWS = 512                                                      # score_candidates' default max_rows


def median(xs):
    return sorted(xs)[len(xs) // 2]


def plan(n):
    a = decode.AnswerSet(synth.make_answer_set(n, V, seed=n), vocab=V)
    lv = a.levels()
    chunk = min(n, max(1, SCORE_ROWS // B))
    forced = -(-n // chunk) * chunk * B * (a.max_len + 1)             # every chunk has `chunk` candidates per sample and runs Lmax + 1 steps
    return a, {"answers": n, "max_len": a.max_len, "nodes": a.n_nodes, "levels": [lv.level_ptr[d + 1] - lv.level_ptr[d] for d in range(lv.depth_max + 1)],
               "decoder_rows": {"rank_candidates": B * a.n_nodes, "score_candidates": forced}}


sets = {n: plan(n) for n in (1500, 3129)}
res = {"batch": B, "frames": 8, "audio_slices": 2, "group": "tva", "vocab": V,
       "sets": {f"shared_{n}": info for n, (_, info) in sets.items()}}
if RESUME and os.path.exists(OUT):
    old = json.load(open(OUT))
    if any(old.get(k) != v for k, v in res.items()):
        sys.exit(f"answer_rank_bench: {OUT} holds another geometry")
    res = old
if PLAN:
    print(json.dumps(res, indent=1))
    sys.exit(0)
if not torch.cuda.is_available():
    sys.exit("answer_rank_bench: no GPU (a timing needs one; --plan prints the row counts)")

from valor_amd.model.valor import VALOR  # noqa: E402

dev = torch.device("cuda:0")
spec = synth.base_spec()
batch = synth.make_batch(spec, batch=B, frames=8, audio_slices=2, txt_len=32, seed=50, questions=True)
batch["video_pixels"] = batch["video_pixels"].to(dev)
batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)


def timed(fn):
    """(seconds, the allocator's peak in GiB, the result) of one call that ends in a device synchronise"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2 ** 30, out


def kernel_us(a, nodes, b):
    """one launch on nodes x b = 8192 rows (max_rows) of the padded logits; nodes: positions in breadth-first order"""
    trie, lv = a.device(dev), a.levels(dev)
    level = lv.order[nodes[0]:nodes[1]].contiguous()
    rows = level.numel() * b
    edges = int((a.child_ptr[1:] - a.child_ptr[:-1])[a.levels().order[nodes[0]:nodes[1]].long()].sum()) * b
    logits = torch.zeros((rows, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :V]
    logits.copy_(torch.randn((rows, V), generator=torch.Generator().manual_seed(1)).to(dev) * 2)
    ns = torch.zeros(a.n_nodes * b, dtype=torch.float32, device=dev)
    fin = torch.zeros(a.n_nodes * b, dtype=torch.float32, device=dev)
    lse = decode.row_lse(logits)[0]
    out = {}
    for name, kw in (("lse_in_the_launch", {}), ("lse_handed_in", {"lse": lse})):
        go = lambda: K.trie_score_level(logits, level, b, decode.EOS, trie, ns, fin, **kw)
        for _ in range(5):
            go()
        times = []
        for _ in range(15):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                go()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / 10)
        out[name + "_us"] = round(median(times), 1)
    out["rows"], out["row_bytes"], out["b"], out["edge_stores"] = rows, V * 4, b, edges
    out["lse_in_the_launch_GBps"] = round(rows * V * 4 / out["lse_in_the_launch_us"] / 1e3, 1)
    return out


def save():
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)


def note(text):
    print(f"[answer_rank_bench] {text}", file=sys.stderr, flush=True)


with torch.no_grad():
    # every row on the root (the edge stores at their most: each row scores the root's ~1200 children), and what a chunk of the pass
    # looks like: 128 nodes of level 1 for 64 samples (a child or none per node)
    for key, nodes, b in (("trie_score_level_root_3129", (0, 1), 8192), ("trie_score_level_level1_3129", (1, 129), 64)):
        if key not in res:
            res[key] = kernel_us(sets[3129][0], nodes, b)
            note(f"{key}: {json.dumps(res[key])}")
            save()
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        todo = [n for n in sets if f"shared_{n}" not in res.get(name, {})]
        if not todo:
            continue
        model = VALOR({"dropout": 0.1, "max_generation_len": 10}, spec=spec, dtype=dtype, device=dev)
        model.load_state_dict(synth.make_state_dict(spec, seed=50), strict=True)
        model.eval()
        prompt = model.qa_prompt(batch["question_tokens"]["bert_tokens"].cpu())
        res["prompt_slots"] = int(prompt.shape[1])
        out = res.setdefault(name, {})
        for n in todo:
            a = sets[n][0]
            run = {"rank_candidates": lambda: decode.rank_candidates(model, batch, ["tva"], a, prompt_cpu=prompt)["tva"],
                   "score_candidates": lambda: decode.score_candidates(model, batch, ["tva"], a, prompt_cpu=prompt)["tva"]}
            last = {}
            for k in run:                                              # warm-up: code objects, the session's capture, GEMM choices
                t, _, last[k] = timed(run[k])
                note(f"{name} shared_{n} {k} warm-up {t:.2f} s")
            diff = float((last["rank_candidates"] - last["score_candidates"]).abs().max())
            times, peak = {k: [] for k in run}, {k: 0.0 for k in run}
            for _ in range(ROUNDS):
                for k in run:
                    t, p, _ = timed(run[k])
                    note(f"{name} shared_{n} {k} {t:.2f} s")
                    times[k].append(t)
                    peak[k] = max(peak[k], p)
            cell = out[f"shared_{n}"] = {"max_abs_score_difference": diff, "top1_agree": int((last["rank_candidates"].argmax(1) ==
                                                                                              last["score_candidates"].argmax(1)).sum())}
            for k in run:
                cell[k] = {"seconds": round(median(times[k]), 4), "questions_per_s": round(B / median(times[k]), 2),
                           "runs_s": [round(x, 4) for x in times[k]], "peak_GiB": round(peak[k], 2)}
            cell["score_over_rank"] = round(median(times["score_candidates"]) / median(times["rank_candidates"]), 2)
            note(f"{name} shared_{n}: {json.dumps(cell)}")
            save()
            del last
        del model
        torch.cuda.empty_cache()
print(json.dumps(res))
save()
