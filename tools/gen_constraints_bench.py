"""What the generation controls cost: caption generation (decode.generate_cap) at the geometry of the generation figures of DESIGN.md
section 5 -- 64 clips of 8 frames + 2 audio slices, group 'tva', 30 tokens, greedy and beam-3 (random weights never emit [SEP]: every
row runs the full length) -- with the controls off and with no_repeat_ngram_size=3, repetition_penalty=1.2, min_length=5. Both settings
run in ONE process on one kept session, interleaved off / on / off / on ...; a setting's figure is the median of its runs. Also the
time of one valor_logits_constrain launch at the step's shape (R = batch and 3 * batch rows, V = 30522, t = 29) between device events
(20 launches per event pair, the median of 15 pairs).
usage: python tools/gen_constraints_bench.py [out.json] [batch] [max_len] [rounds]      (default profiles/gen_constraints.json 64 30 5)"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from valor_amd import decode, kernels as K, synth  # noqa: E402
from valor_amd.model.valor import VALOR  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gen_constraints.json")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
L = int(sys.argv[3]) if len(sys.argv) > 3 else 30
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
ON = {"no_repeat_ngram_size": 3, "repetition_penalty": 1.2, "min_length": 5}
dev = torch.device("cuda:0")
spec = synth.base_spec()
model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device=dev)
model.load_state_dict(synth.make_state_dict(spec, seed=50), strict=True)
batch = synth.make_batch(spec, batch=B, frames=8, audio_slices=2, txt_len=32, seed=50)
batch["video_pixels"] = batch["video_pixels"].to(dev)
batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
res = {"batch": B, "frames": 8, "audio_slices": 2, "max_generation_len": L, "group": "tva", "rounds": ROUNDS, "on": ON}


def seconds(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def median(xs):
    return sorted(xs)[len(xs) // 2]


def launch_us(R, V, t):
    logits = torch.zeros((R, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :V]
    logits.copy_(torch.randn((R, V), generator=torch.Generator().manual_seed(V)) * 2)
    hist = torch.randint(1000, 1000 + 12, (R, t + 1), generator=torch.Generator().manual_seed(t)).to(dev)
    c = decode.Constraints(**ON)
    go = lambda: K.logits_constrain(logits, hist, t, decode.EOS, c.penalty, c.inv_penalty, c.no_repeat_ngram_size, c.min_length)
    for _ in range(10):
        go()
    times = []
    for _ in range(15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            go()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / 20)
    return round(median(times), 2)


with torch.no_grad():
    model.eval()
    enc = [seconds(lambda: decode.encode_for_generation(model, batch, ["tva"])) for _ in range(4)]
    res["encode_ms"] = round(median(enc[1:]) * 1e3, 1)
    for name, beam in (("greedy", 1), ("beam3", 3)):
        run = {"off": lambda: decode.generate_cap(model, batch, ["tva"], beam_size=beam, max_generation_len=L),
               "on": lambda: decode.generate_cap(model, batch, ["tva"], beam_size=beam, max_generation_len=L, **ON)}
        for k in ("off", "on"):                              # first runs: the session, its eager step and the capture
            run[k]()
        times = {"off": [], "on": []}
        for _ in range(ROUNDS):
            for k in ("off", "on"):
                times[k].append(seconds(run[k]))
        out = res[name] = {}
        for k in ("off", "on"):
            t = median(times[k])
            out[k] = {"seconds": round(t, 4), "captions_per_s": round(B / t, 1), "ms_per_decoding_step": round((t * 1e3 - res["encode_ms"]) / L, 3),
                      "runs_s": [round(x, 4) for x in times[k]]}
        out["on_over_off"] = round(median(times["on"]) / median(times["off"]), 4)
        out["extra_us_per_step"] = round((median(times["on"]) - median(times["off"])) * 1e6 / L, 1)
    res["constrain_launch_us"] = {f"R{R}_V30522_t{L - 1}": launch_us(R, 30522, L - 1) for R in (B, 3 * B)}
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(res, open(OUT, "w"), indent=1)
