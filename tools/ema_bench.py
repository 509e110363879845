"""What weight averaging (valor_amd/ema.py) costs at the benchmark's base configuration (VALOR-base, CLIP variant, b = 64, 8 frames, 2 audio
slices, bf16 + fp32 masters, dropout 0.1, graphs as the engine defaults them), in ONE process:
  * the step: train_step with the engine's average off (ema_decay 0) and on (ema_decay 0.9999, every step), interleaved span by span on
    the same engine -- host-clock spans around `iters` optimizer steps that end in a device synchronise, medians over `reps`;
  * the kernel alone: valor_ema_update over the arena (12 B per parameter: read w, read ema, write ema) for every setting of its
    non-temporal hook (valor_ema_set_nt: 0 none, 1 loads, 2 stores, 3 both), and valor_adamw_counted over the same arena (28 B per
    parameter: master, both moments read and written, the bf16 gradient read, the bf16 parameter written; zero_grad off) -- device
    events around `kernel_iters` back-to-back launches, the settings interleaved over `reps` rounds, medians. Both kernels stream
    memory, so their byte rates are comparable.
Writes profiles/ema_bench.json.

    python tools/ema_bench.py [--reps 5] [--iters 5] [--kernel-iters 20] [--batch 64] [--out profiles/ema_bench.json]
"""
import argparse
import ctypes
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="optimizer steps per timed span")
    ap.add_argument("--kernel-iters", type=int, default=20, help="launches per timed kernel span")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--audio-slices", type=int, default=2)
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--tiny", action="store_true", help="the unit-test architecture instead of VALOR-base (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_bench.py measures on the GPU: none found")
    from valor_amd import lib, synth
    from valor_amd.ema import WeightEMA
    from valor_amd.engine import TrainEngine
    from valor_amd.kernels import _ptr, _stream, dt_of
    from valor_amd.model.valor import VALOR
    dev = torch.device("cuda:0")
    spec = synth.tiny_spec() if args.tiny else synth.base_spec()
    model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device=dev)
    sd = synth.make_state_dict(spec, seed=50)
    model.load_state_dict(sd, strict=True)
    opts = SimpleNamespace(learning_rate=1e-4, weight_decay=0.01, clip_lr=5e-7, clip_lr_text=5e-7, new_lr=0.0, decoder_lr=-1, betas=[0.9, 0.98],
                           warmup_ratio=0.1, num_train_steps=100000, scheduler="warmup_linear", grad_norm=5.0)
    eng = TrainEngine(model, opts)
    opt = eng.optimizer
    opt.init_master_from(sd)
    del sd
    ema = WeightEMA(opt, args.decay)
    batch = synth.make_batch(spec, batch=args.batch, frames=args.frames, audio_slices=args.audio_slices, txt_len=32, seed=50)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    n = model.arena.numel

    # ---- the step, average off / on
    def span(with_ema):
        eng.ema = ema if with_ema else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            eng.train_step(batch, TASK)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    for on in (False, True, False, True):               # allocations, graph captures, the allocator's head-room
        for _ in range(3):
            span(on)
    step = {"off": [], "on": []}
    for _ in range(args.reps):
        step["off"].append(span(False))
        step["on"].append(span(True))
    eng.ema = None
    updates = ema.updates

    # ---- the kernels alone
    a = model.arena
    table = opt._table(list(a.offsets))
    lr = (ctypes.c_float * opt.N_GROUPS)(*[g["lr"] for g in opt.param_groups])
    wd = (ctypes.c_float * opt.N_GROUPS)(*[g["weight_decay"] for g in opt.param_groups])
    opt.gscale.fill_(1.0)
    a.grad.zero_()

    def launch_ema():
        lib.call("valor_ema_update", _stream(), _ptr(opt.master), _ptr(ema.ema), n, ema.decay, 1, _ptr(ema.count), _ptr(opt.gscale))

    def launch_adamw():
        lib.call("valor_adamw_counted", _stream(), dt_of(a.grad), _ptr(opt.master), _ptr(opt.exp_avg), _ptr(opt.exp_avg_sq), _ptr(a.grad),
                 _ptr(a.flat), _ptr(table), _ptr(opt._chunk_tensor), _ptr(opt._count), opt._count.numel(), _ptr(opt._chunk_bc), n, lr, wd,
                 opt.N_GROUPS, opt.betas[0], opt.betas[1], opt.eps, 1, _ptr(opt.gscale), 0)

    def kspan(fn):
        for _ in range(3):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.kernel_iters):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / args.kernel_iters

    so = lib.load()
    default_nt = so.valor_ema_set_nt(-1)
    kms = {f"ema_nt{v}": [] for v in range(4)}
    kms["adamw_counted"] = []
    for _ in range(args.reps):
        for v in range(4):
            so.valor_ema_set_nt(v)
            kms[f"ema_nt{v}"].append(kspan(launch_ema))
        kms["adamw_counted"].append(kspan(launch_adamw))
    so.valor_ema_set_nt(default_nt)
    med = {k: statistics.median(v) for k, v in kms.items()}
    rate = lambda ms, bytes_per: n * bytes_per / (ms * 1e-3) / 1e12
    soff, son = statistics.median(step["off"]), statistics.median(step["on"])
    res = {"config": {"variant": "tiny" if args.tiny else "clip", "batch": args.batch, "frames": args.frames, "audio_slices": args.audio_slices,
                      "dtype": "bf16", "dropout": 0.1, "graphs": bool(model._graphs_on), "task": TASK, "decay": args.decay, "reps": args.reps,
                      "iters": args.iters, "kernel_iters": args.kernel_iters, "arena_numel": n},
           "step_ms": {k: {"median": round(statistics.median(v), 3), "all": [round(x, 3) for x in v]} for k, v in step.items()},
           "ema_step_cost_ms": round(son - soff, 3), "ema_share_of_step": round((son - soff) / son, 5), "ema_updates_during_steps": updates,
           "kernel": {k: {"ms": round(med[k], 4), "tb_per_s": round(rate(med[k], 28 if k == "adamw_counted" else 12), 3),
                          "all_ms": [round(x, 4) for x in kms[k]]} for k in kms},
           "default_nt": default_nt,
           "ema_over_adamw_byte_rate": round(rate(med[f"ema_nt{default_nt}"], 12) / rate(med["adamw_counted"], 28), 3),
           "kernel_share_of_step": round(med[f"ema_nt{default_nt}"] / son, 5)}
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
