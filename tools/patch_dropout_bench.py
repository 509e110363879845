"""What video patch dropout buys at the benchmark's base configuration (BASELINE configs[1]: VALOR-base, CLIP variant, batch 64, 8 frames,
2 audio slices, bf16 + fp32 masters, dropout 0.1, graphs on): training steps at rate 0 (the path without the option), 0.25, 0.5 and 0.75,
and at video_patch_keep = 95 (S' = 96 rows per frame) beside rate 0.5 (S' = 99), in ONE process on one model and engine whose kept count
is switched. All variants are warmed up first (graph captures included), then they alternate: a round times `iters` steps of each in
turn, each span behind `rewarm` untimed steps. A step time comes from two device events around a synchronised span. Ratios are taken against
rate 0 of the SAME round; the spread over the rounds is reported with them. The ViT rows and cross K|V rows per clip come from the shapes.
Writes profiles/patch_dropout_bench.json.

    python tools/patch_dropout_bench.py [--reps 5] [--iters 3] [--batch 64] [--mode frame] [--out profiles/patch_dropout_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
VARIANTS = (("rate_0", {}), ("rate_0.25", {"video_patch_dropout": 0.25}), ("rate_0.5", {"video_patch_dropout": 0.5}),
            ("keep_95", {"video_patch_keep": 95}), ("rate_0.75", {"video_patch_dropout": 0.75}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="rounds over the variants")
    ap.add_argument("--iters", type=int, default=3, help="training steps per timed span")
    ap.add_argument("--warmup", type=int, default=5, help="steps of every variant ahead of the first round (graphs capture on the third)")
    ap.add_argument("--rewarm", type=int, default=3, help="untimed steps after every switch of the variant (the decoder's graph is captured on the third)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--audio-slices", type=int, default=2)
    ap.add_argument("--mode", default="frame", choices=("frame", "tube"))
    ap.add_argument("--variants", default=",".join(n for n, _ in VARIANTS), help="a subset of the variants (rate_0 is always measured)")
    ap.add_argument("--tiny", action="store_true", help="the unit-test architecture instead of VALOR-base (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_dropout_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/patch_dropout_bench.py measures on the GPU: none found")
    from valor_amd import synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR, patch_keep_count
    dev = torch.device("cuda:0")
    spec = synth.tiny_spec() if args.tiny else synth.base_spec()
    Pn = spec.vis_tokens - 1
    wanted = set(args.variants.split(",")) | {"rate_0"}
    unknown = wanted - {n for n, _ in VARIANTS}
    if unknown:
        raise SystemExit(f"--variants: unknown {sorted(unknown)}")
    sd = synth.make_state_dict(spec, seed=50)
    batch = synth.make_batch(spec, batch=args.batch, frames=args.frames, audio_slices=args.audio_slices, txt_len=32, seed=50)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    opts = SimpleNamespace(learning_rate=1e-4, weight_decay=0.01, clip_lr=5e-7, clip_lr_text=5e-7, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100000, scheduler="warmup_linear", grad_norm=5.0)
    # ONE model and engine (the gradient-write listener of the reducer is per process): a variant is the model's kept count. The ViT keeps a
    # captured graph per variant (graph key: shape + kept count); the decoder stack's static K|V buffers follow the row count, so a switch
    # releases them with the decoder's graph -- every span is therefore preceded by `--rewarm` untimed steps that capture it again.
    os.environ.setdefault("VALOR_GRAPH_MAX_KEYS", "8")
    model = VALOR({"dropout": 0.1, "video_patch_dropout_mode": args.mode, "video_patch_keep": Pn - 1}, spec=spec, dtype=torch.bfloat16, device=dev)
    model.load_state_dict(sd, strict=True)
    eng = TrainEngine(model, opts, graphs=True)
    eng.optimizer.init_master_from(sd)
    del sd
    runs = []
    for name, o in VARIANTS:
        if name not in wanted:
            continue
        if args.tiny and "video_patch_keep" in o:
            o = {"video_patch_keep": max(1, Pn // 2 - 1)}
        k = patch_keep_count(Pn, o.get("video_patch_dropout", 0.0), o.get("video_patch_keep"))
        rows = {"kept_patches": k, "tokens_per_frame": 1 + k, "vit_rows_per_clip": args.frames * (1 + k),
                "cross_kv_rows_per_clip": args.frames * (1 + k) + args.audio_slices * spec.aud_tokens}
        print(f"[patch_dropout_bench] {name}: {rows}", flush=True)
        runs.append({"name": name, "keep": k if k < Pn else None, "rows": rows, "ms": [], "loss": None, "graphs": None})

    def span(r, n):
        model.patch_keep = r["keep"]                          # None: the path without the option
        for _ in range(args.rewarm):
            eng.train_step(batch, TASK)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            out = eng.train_step(batch, TASK)
        e1.record()
        torch.cuda.synchronize()
        r["loss"] = {k: round(float(v.detach()), 4) for k, v in out.items()}
        r["graphs"] = {n_: len(s.captured) for n_, s in model._graph_segs.items()}
        return e0.elapsed_time(e1) / n

    for r in runs:                                            # every shape of the timed spans, graph captures included
        span(r, args.warmup)
    for _ in range(args.reps):                                # the variants alternate
        for r in runs:
            r["ms"].append(span(r, args.iters))
    base = runs[0]
    res = {"config": {"variant": "tiny" if args.tiny else "clip", "batch": args.batch, "frames": args.frames, "audio_slices": args.audio_slices,
                      "dtype": "bf16", "dropout": 0.1, "graphs": True, "mode": args.mode, "task": TASK, "reps": args.reps, "iters": args.iters, "rewarm": args.rewarm,
                      "timing": "device events around a synchronised span of `iters` steps; ratios against rate_0 of the same round"},
           "variants": {}}
    for r in runs:
        med = statistics.median(r["ms"])
        ratio = [b / m for m, b in zip(r["ms"], base["ms"])]                  # > 1: faster than rate 0
        res["variants"][r["name"]] = dict(
            r["rows"],
            step_ms={"median": round(med, 2), "all": [round(x, 2) for x in r["ms"]]},
            steps_per_s=round(1e3 / med, 3), samples_per_s=round(args.batch * 1e3 / med, 1),
            speedup_over_rate_0={"median": round(statistics.median(ratio), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)},
            vit_rows_over_rate_0=round(r["rows"]["vit_rows_per_clip"] / base["rows"]["vit_rows_per_clip"], 4),
            graphs_captured=r["graphs"],
            last_losses=r["loss"])
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
