"""What a checkpoint costs the training step at the benchmark's base configuration (VALOR-base, CLIP variant, B = 64, 8 frames, 2 audio
slices, bf16 + fp32 masters, dropout 0.1): the device-side period of the step that follows a save -- the time between the `tail` events
(TrainEngine.trace) of the step before the save and of the step after it, which contains whatever the save put on the stream or kept the
host from issuing -- for no save, save_run(blocking=True) and save_run(blocking=False), in ONE process, interleaved; and the wall time
from the call until the files are complete (SaveHandle.seconds). Writes profiles/ckpt_bench.json.

    python tools/ckpt_bench.py [--reps 3] [--batch 64] [--dir /some/scratch] [--out profiles/ckpt_bench.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--audio-slices", type=int, default=2)
    ap.add_argument("--settle", type=int, default=4, help="plain steps between two saves (they are the no-save samples)")
    ap.add_argument("--dir", default=None, help="where the checkpoints go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ckpt_bench.json"))
    args = ap.parse_args()
    from valor_amd import checkpoint, synth
    from valor_amd.engine import TrainEngine
    from valor_amd.model.valor import VALOR
    dev = torch.device("cuda:0")
    spec = synth.base_spec()
    model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device=dev)
    sd = synth.make_state_dict(spec, seed=50)
    model.load_state_dict(sd, strict=True)
    opts = SimpleNamespace(learning_rate=1e-4, weight_decay=0.01, clip_lr=5e-7, clip_lr_text=5e-7, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100000, scheduler="warmup_linear", grad_norm=5.0)
    eng = TrainEngine(model, opts)
    eng.optimizer.init_master_from(sd)
    del sd
    batch = synth.make_batch(spec, batch=args.batch, frames=args.frames, audio_slices=args.audio_slices, txt_len=32, seed=50)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    out_dir = args.dir or tempfile.mkdtemp(prefix="valor_ckpt_bench_")
    for _ in range(6):
        eng.train_step(batch, TASK)
    t0 = time.perf_counter()
    first = checkpoint.save_run(eng, out_dir, blocking=False)           # allocates the snapshot and pinned buffers: not a sample
    eng.train_step(batch, TASK)
    first.wait()
    first_call_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    eng.trace = []
    marks, handles, exclude = [], [], set()  # marks: (index into the trace of the step issued right after the save, mode)
    for _ in range(args.reps):
        for mode in ("blocking", "non_blocking"):
            if handles:
                handles[-1][1].wait()       # the writer of the previous sample is done before this one starts: its wait is not this save's cost
                exclude.add(len(eng.trace))
            for _ in range(args.settle):
                eng.train_step(batch, TASK)
            h = checkpoint.save_run(eng, out_dir, blocking=mode == "blocking")
            marks.append((len(eng.trace), mode))
            exclude.update((len(eng.trace), len(eng.trace) + 1))
            eng.train_step(batch, TASK)
            handles.append((mode, h))
    for _ in range(args.settle):
        eng.train_step(batch, TASK)
    for _, h in handles:
        h.wait()
    torch.cuda.synchronize()
    tr = eng.trace
    period = [None] + [tr[i - 1]["tail"].elapsed_time(tr[i]["tail"]) for i in range(1, len(tr))]
    # no-save samples: not the step that follows a save, not the one after it (the side stream may still be copying), not one that
    # follows a host-side wait for the writer
    plain = [p for i, p in enumerate(period) if p is not None and i not in exclude]
    res = {"config": {"variant": "clip", "batch": args.batch, "frames": args.frames, "audio_slices": args.audio_slices, "dtype": "bf16",
                      "graphs": bool(model._graphs_on), "reps": args.reps},
           "bytes": {"parameters": model.arena.flat.numel() * model.arena.flat.element_size(), "fp32_state": 3 * eng.optimizer.master.numel() * 4},
           "first_non_blocking_save_s": round(first_call_s, 3),
           "step_period_ms": {"no_save": {"median": round(statistics.median(plain), 2), "min": round(min(plain), 2), "max": round(max(plain), 2),
                                          "n": len(plain)}},
           "files_complete_s": {}}
    for mode in ("blocking", "non_blocking"):
        ps = [period[i] for i, m in marks if m == mode]
        res["step_period_ms"][mode] = {"median": round(statistics.median(ps), 2), "all": [round(p, 2) for p in ps]}
        secs = [h.seconds for m, h in handles if m == mode]
        res["files_complete_s"][mode] = {"median": round(statistics.median(secs), 3), "all": [round(s, 3) for s in secs]}
    ns, b, nb = (res["step_period_ms"][k]["median"] for k in ("no_save", "blocking", "non_blocking"))
    res["non_blocking_closer_to_no_save_than_to_blocking"] = bool(abs(nb - ns) < abs(b - nb))
    eng.close()
    if args.dir is None:
        shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
