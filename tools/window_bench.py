"""What the window step costs at the benchmark's base configuration (VALOR-base, CLIP variant, b = 64 per micro-batch, 8 frames, 2 audio
slices, bf16 + fp32 masters, dropout 0.1, graphs as the engine defaults them): for M = 2 and M = 4 micro-batches, in ONE process and
interleaved,
  * plain accumulation: M x train_step(accum_steps=M) -- M contrastive matrices of 64 rows;
  * the window step: train_window on the same M micro-batches -- one contrastive evaluation over N = 64 M rows;
  * the feature pass of the window step alone (TrainEngine.feature_pass).
Times are host-clock spans around `iters` optimizer steps that end in a device synchronise; the medians over `reps` go into the file.
The expected gap between the first two is the third (one extra encoder forward per micro-batch, run eagerly and without autograd);
`unexplained_ms` is what is left. Writes profiles/window_contrastive_bench.json.

    python tools/window_bench.py [--reps 3] [--iters 3] [--batch 64] [--windows 2,4] [--out profiles/window_contrastive_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3, help="optimizer steps per timed span")
    ap.add_argument("--batch", type=int, default=64, help="rows per micro-batch")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--audio-slices", type=int, default=2)
    ap.add_argument("--windows", default="2,4")
    ap.add_argument("--tiny", action="store_true", help="the unit-test architecture instead of VALOR-base (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_contrastive_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/window_bench.py measures on the GPU: none found")
    from valor_amd import synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    dev = torch.device("cuda:0")
    spec = synth.tiny_spec() if args.tiny else synth.base_spec()
    model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device=dev)
    sd = synth.make_state_dict(spec, seed=50)
    model.load_state_dict(sd, strict=True)
    opts = SimpleNamespace(learning_rate=1e-4, weight_decay=0.01, clip_lr=5e-7, clip_lr_text=5e-7, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100000, scheduler="warmup_linear", grad_norm=5.0)
    eng = TrainEngine(model, opts)
    eng.optimizer.init_master_from(sd)
    del sd
    # largest window first, each a multiple of the next: train_step closes an accumulation window on every accum_steps-th call of the
    # engine's life, so the calls made for one M must leave the count aligned for the next
    windows = sorted((int(w) for w in args.windows.split(",")), reverse=True)
    if any(a % b for a, b in zip(windows, windows[1:])):
        raise SystemExit(f"--windows {args.windows}: every window size must divide the next larger one")
    batches = []
    for m in range(max(windows)):
        b = synth.make_batch(spec, batch=args.batch, frames=args.frames, audio_slices=args.audio_slices, txt_len=32, seed=50 + m)
        b["video_pixels"] = b["video_pixels"].to(dev)
        b["audio_spectrograms"] = b["audio_spectrograms"].to(dev)
        batches.append(b)

    def accum(M):
        for m in range(M):
            out = eng.train_step(batches[m], TASK, accum_steps=M)
        return out

    def window(M):
        return eng.train_window(batches[:M], TASK)

    def features(M):
        eng.feature_pass(batches[:M], TASK)

    def span(fn, M):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn(M)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    res = {"config": {"variant": "tiny" if args.tiny else "clip", "micro_batch": args.batch, "frames": args.frames,
                      "audio_slices": args.audio_slices, "dtype": "bf16", "dropout": 0.1, "graphs": bool(model._graphs_on), "task": TASK,
                      "reps": args.reps, "iters": args.iters},
           "windows": {}}
    for M in windows:
        for fn in (accum, window, features):              # every shape and path of the timed spans, graph captures included
            for _ in range(4):
                fn(M)
        ms = {"accum": [], "window": [], "features": []}
        for _ in range(args.reps):
            ms["accum"].append(span(accum, M))
            ms["window"].append(span(window, M))
            ms["features"].append(span(features, M))
        losses = {k: round(float(v), 4) for k, v in window(M).items()}
        own = round(float(accum(M)["contra_loss"].detach()), 4)
        med = {k: statistics.median(v) for k, v in ms.items()}
        N = M * args.batch
        res["windows"][str(M)] = {
            "rows": N,
            "step_ms": {k: {"median": round(med[k], 2), "all": [round(x, 2) for x in v]} for k, v in ms.items()},
            "samples_per_s": {"accum": round(N / med["accum"] * 1e3, 1), "window": round(N / med["window"] * 1e3, 1)},
            "window_over_accum": round(med["window"] / med["accum"], 4),
            "feature_pass_share_of_window": round(med["features"] / med["window"], 4),
            "unexplained_ms": round(med["window"] - med["accum"] - med["features"], 2),
            "window_losses": losses,
            "last_micro_batch_own_contra_loss": own,
        }
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
