"""What the training diagnostics cost: the headline step (bench.py's configuration: VALOR-base, bf16, batch 64) as a bare loop of
engine.train_step calls, interleaved off / level 'grad' / level 'full' / off in one process on one engine, then the two entry points alone
(valor_arena_grad_stats, valor_arena_update_stats on the live arenas, timed with events) for their achieved bandwidth. Prints ms per
step of the four runs, the off / off spread as the noise floor, what each level adds over the mean of the two off runs, and per entry
point (three launches: the streaming pass and two small reductions) microseconds, bytes read and TB/s; writes the JSON (default profiles/diagnostics_bench.json).

    python tools/diagnostics_bench.py --steps 30 --warmup 8 [--batch 64] [--out FILE]"""
import argparse
import json
import os
import random
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--audio-slices", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics_bench.json"))
    args = ap.parse_args()

    from valor_amd import synth
    from valor_amd.diagnostics import Diagnostics
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    from valor_amd.ops import DropoutState
    dev = torch.device("cuda:0")
    spec = synth.base_spec()
    np.random.seed(50)
    model = VALOR({"dropout": 0.1, "checkpointing": False}, spec=spec, dtype=torch.bfloat16, device=dev)
    sd = synth.make_state_dict(spec, seed=50)
    model.load_state_dict(sd, strict=True)
    opts = SimpleNamespace(learning_rate=1e-4, weight_decay=0.01, clip_lr=5e-7, clip_lr_text=5e-7, new_lr=0.0, decoder_lr=-1,
                           betas=[0.9, 0.98], warmup_ratio=0.1, num_train_steps=100000, scheduler="warmup_linear", grad_norm=5.0)
    engine = TrainEngine(model, opts)
    opt = engine.optimizer
    opt.init_master_from(sd)
    del sd
    batch = synth.make_batch(spec, batch=args.batch, frames=args.frames, audio_slices=args.audio_slices, txt_len=32, seed=50)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    random.seed(50)
    DropoutState.reset(1234)
    levels = {"grad": Diagnostics(opt, level="grad"), "full": Diagnostics(opt, level="full")}

    def run(level, n):
        engine.diagnostics = levels.get(level)
        for _ in range(n):
            engine.train_step(batch, TASK)

    def timed(level):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(level, args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return {"ms_per_step": round(el * 1e3 / args.steps, 3), "samples_per_s": round(args.steps * args.batch / el, 2)}

    run(None, args.warmup)
    run("grad", 2)
    run("full", 2)
    runs = {"off1": timed(None), "grad": timed("grad"), "full": timed("full"), "off2": timed(None)}
    engine.diagnostics = None
    off = 0.5 * (runs["off1"]["ms_per_step"] + runs["off2"]["ms_per_step"])

    # the entry points alone, on the arenas as the last step left them (the gradient arena is clear: the traffic is the same)
    a, diag = opt.arena, levels["full"]
    table = opt._table(list(a.offsets))
    lr = [g["lr"] for g in opt.param_groups]

    def kernel(fn, between, nbytes):
        # `between` runs in front of every timed call and streams 4.5 GB (or 0.75 GB) of other data: without it repeated calls find a
        # third of the 0.75 GB gradient arena in the 256 MB last-level cache and report a bandwidth no training step sees
        fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.kernel_reps)]
        for a0, a1 in ev:
            between()
            a0.record()
            fn()
            a1.record()
        torch.cuda.synchronize()
        us = sorted(a0.elapsed_time(a1) * 1e3 for a0, a1 in ev)
        med = us[len(us) // 2]
        return {"us_median": round(med, 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1), "bytes_read": int(nbytes),
                "tb_per_s": round(nbytes / med / 1e6, 3)}

    grad_stats, update_stats = (lambda: diag.grad_stats(table, 1.0)), (lambda: diag.update_stats(table, lr))
    kernels = {"valor_arena_grad_stats": kernel(grad_stats, update_stats, a.numel * a.grad.element_size()),
               "valor_arena_update_stats": kernel(update_stats, grad_stats, a.numel * 12)}
    out = {"bench": "diagnostics", "batch": args.batch, "frames": args.frames, "audio_slices": args.audio_slices, "steps": args.steps,
           "warmup": args.warmup, "arena_elements": int(a.numel), "tensors": len(a.offsets), "runs": runs,
           "off_off_spread_ms": round(abs(runs["off1"]["ms_per_step"] - runs["off2"]["ms_per_step"]), 3),
           "grad_adds_ms": round(runs["grad"]["ms_per_step"] - off, 3), "full_adds_ms": round(runs["full"]["ms_per_step"] - off, 3),
           "kernels": kernels, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    engine.close()


if __name__ == "__main__":
    main()
