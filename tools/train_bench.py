"""What the training driver costs: (A) the bare loop of engine.train_step calls as bench.py times the headline step, (B) Trainer.fit on
the same batches (log_every = 200, no validation, the device meter fed every step), interleaved A, B, A in one process on one engine.
Prints samples/s of the three runs, the host's busy time per step (call-to-call time minus the time blocked in the engine's throttle) and
the A/A difference, and writes the JSON (default profiles/train_driver_bench.json).

The condition: B is not below the slower of the two A runs by more than the A/A difference of the same process.

    python tools/train_bench.py --steps 30 --warmup 8 [--batch 64] [--out FILE]"""
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


class Repeat:
    """the benchmark's loader: one device-resident batch under one name, endlessly"""
    ndata = 1

    def __init__(self, name, batch):
        self.item = (name, batch)

    def __iter__(self):
        while True:
            yield self.item


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--audio-slices", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_driver_bench.json"))
    args = ap.parse_args()

    from valor_amd import synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    from valor_amd.ops import DropoutState
    from valor_amd.train import Trainer
    dev = torch.device("cuda:0")
    spec = synth.base_spec()
    np.random.seed(50)
    model = VALOR({"dropout": 0.1, "checkpointing": False}, spec=spec, dtype=torch.bfloat16, device=dev)
    sd = synth.make_state_dict(spec, seed=50)
    model.load_state_dict(sd, strict=True)
    opts = SimpleNamespace(learning_rate=1e-4, weight_decay=0.01, clip_lr=5e-7, clip_lr_text=5e-7, new_lr=0.0, decoder_lr=-1,
                           betas=[0.9, 0.98], warmup_ratio=0.1, num_train_steps=100000, scheduler="warmup_linear", grad_norm=5.0)
    engine = TrainEngine(model, opts)
    engine.optimizer.init_master_from(sd)
    del sd
    batch = synth.make_batch(spec, batch=args.batch, frames=args.frames, audio_slices=args.audio_slices, txt_len=32, seed=50)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    random.seed(50)
    DropoutState.reset(1234)

    entered, inner = [], engine.train_step

    def stamped(b, task, accum_steps=1):
        entered.append(time.perf_counter())
        return inner(b, task, accum_steps=accum_steps)
    engine.train_step = stamped

    def bare(n):
        for _ in range(n):
            engine.train_step(batch, TASK)

    trainer = Trainer(engine, Repeat(TASK + "--bench", batch), log_fn=lambda step, scalars: None, log_every=200)

    def driver(n):
        trainer.num_train_steps = engine.global_step + n          # the LR schedule keeps opts.num_train_steps
        trainer.fit()

    def timed(fn):
        torch.cuda.synchronize()
        del entered[:]
        engine.trace = []
        t0 = time.perf_counter()
        fn(args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        trace, engine.trace = engine.trace, None
        wait = sum(r["wait_ms"] for r in trace[1:]) / max(len(trace) - 1, 1)
        call = (entered[-1] - entered[0]) * 1e3 / max(len(entered) - 1, 1)
        return {"samples_per_s": round(args.steps * args.batch / el, 2), "ms_per_step": round(el * 1e3 / args.steps, 3),
                "host_busy_ms_per_step": round(call - wait, 3), "throttle_wait_ms_per_step": round(wait, 3)}

    engine.trace = []
    bare(args.warmup)
    driver(2)                                                     # the meter's first launches, the pinned slot of the final flush
    engine.trace = None
    runs = {"A1": timed(bare), "B": timed(driver), "A2": timed(bare)}
    a1, b, a2 = (runs[k]["samples_per_s"] for k in ("A1", "B", "A2"))
    out = {"bench": "train_driver", "batch": args.batch, "frames": args.frames, "audio_slices": args.audio_slices, "steps": args.steps,
           "warmup": args.warmup, "runs": runs, "aa_difference_samples_per_s": round(abs(a1 - a2), 2),
           "b_below_slower_a_samples_per_s": round(min(a1, a2) - b, 2), "condition_met": bool(min(a1, a2) - b <= abs(a1 - a2)),
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    engine.close()


if __name__ == "__main__":
    main()
