"""Throughput of beam-3 caption generation under the two beam-search rules at the bench geometry (tools/gen_bench.py's: B clips of 8
frames + 2 audio slices, group 'tva', max_generation_len L, random weights -- they never emit [SEP], so every row runs the full length
and neither rule leaves early: the per-step cost is what is compared): generate_cap(beam_search='reference') -- decode_beam, the
parent's code -- against beam_search='pool' (decode_beam_pool: one valor_beam_pool_step launch per step), interleaved in one process,
each measured twice. Reported: captions/s of every run, the spread between the two reference runs, and the pool rule's rate relative to
the reference's mean; the n-best call (num_return_sequences = 3) besides.
usage: python tools/beam_pool_bench.py out.json [batch] [max_len]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from valor_amd import decode, synth  # noqa: E402
from valor_amd.model.valor import VALOR  # noqa: E402

B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
L = int(sys.argv[3]) if len(sys.argv) > 3 else 30
BEAM = 3
dev = torch.device("cuda:0")
spec = synth.base_spec()
model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device=dev)
model.load_state_dict(synth.make_state_dict(spec, seed=50), strict=True)
batch = synth.make_batch(spec, batch=B, frames=8, audio_slices=2, txt_len=32, seed=50)
batch["video_pixels"] = batch["video_pixels"].to(dev)
batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
res = {"batch": B, "frames": 8, "audio_slices": 2, "max_generation_len": L, "group": "tva", "beam": BEAM}


def timed(fn, reps=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


RULES = {"reference": dict(beam_search="reference"), "pool": dict(beam_search="pool"),
         "pool_n_best_3": dict(beam_search="pool", num_return_sequences=BEAM)}
with torch.no_grad():
    model.eval()
    call = {k: (lambda kw=kw: decode.generate_cap(model, batch, ["tva"], beam_size=BEAM, max_generation_len=L, **kw)) for k, kw in RULES.items()}
    for fn in call.values():                               # the session, its captured step and every kernel once
        fn()
    runs = {k: [] for k in RULES}
    for _ in range(2):                                     # interleaved: reference, pool, n-best, and again
        for k in RULES:
            runs[k].append(timed(call[k]))
for k, ts in runs.items():
    res[k] = {"seconds": [round(t, 4) for t in ts], "captions_per_s": [round(B / t, 1) for t in ts],
              "ms_per_token_position": [round(t * 1e3 / L, 3) for t in ts]}
ref = runs["reference"]
ref_mean = sum(ref) / len(ref)
res["reference_spread"] = round(abs(ref[0] - ref[1]) / ref_mean, 4)
res["pool_vs_reference"] = round(ref_mean / (sum(runs["pool"]) / len(runs["pool"])), 4)      # > 1: the pool rule is faster
print(json.dumps(res, indent=1))
json.dump(res, open(sys.argv[1], "w"), indent=1)
