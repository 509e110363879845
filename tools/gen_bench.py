"""Throughput of caption generation (VALOR.generate_cap, model/pretrain.py:914-985) on the native decoder at the bench geometry: B clips of
8 frames + 2 audio slices, group 'tva', greedy and beam-3 decoding to max_generation_len (random weights never emit [SEP]: every row runs
the full length). Prints where the time goes: the encoders + K|V projections (once per clip) and the decoding loop (re-runs the text rows
each step like the reference with VALOR_KV_CACHE=0; two rows per sequence against the K|V cache otherwise, decode.py).
Mode 'sample' is the sampled decode of SCST (decode.decode_sample on the session); mode 'scst' times one self-critical training step at the
caption-msrvtt shape (task cap%tva%tv, a CaptionScorer of 20 synthetic references per clip) split into greedy baseline, encoders +
sampled decoding, scoring and the loss pass (forward + backward), and one scorer call of B hypotheses. GEN_SCORER=host (default) scores
with scst.CaptionScorer on the host, GEN_SCORER=device with scst.DeviceCaptionScorer (valor_caption_reward: one launch for the sample and
greedy rows of both groups, timed up to a device synchronisation); score_ms / scorer_ms_per_call are those of the scorer in use.
Mode 'sampled' is the captioner's sampling: generate_cap(mode='sample') with the filters off, top_k 50, top_p 0.9, temperature 0.7 +
top_k 50 + top_p 0.9, and num_return_sequences 4 at batch / 4 clips (the same number of decoder rows), each as captions/s; and the time
of one sampler launch at R = batch rows, V = 30522 and 49408 -- valor_sample_tokens next to valor_sample_tokens_filtered under the same
settings -- between device events in this process (20 launches per event pair, the median of 15 pairs, after a warm-up).
usage: [GEN_MODES=greedy,beam3,sample,sampled,scst] [GEN_SCORER=host|device] python tools/gen_bench.py out.json [batch] [max_len]"""
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
dev = torch.device("cuda:0")
spec = synth.base_spec()
model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device=dev)
model.load_state_dict(synth.make_state_dict(spec, seed=50), strict=True)
batch = synth.make_batch(spec, batch=B, frames=8, audio_slices=2, txt_len=32, seed=50)
batch["video_pixels"] = batch["video_pixels"].to(dev)
batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
res = {"batch": B, "frames": 8, "audio_slices": 2, "max_generation_len": L, "group": "tva"}


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


MODES = os.environ.get("GEN_MODES", "greedy,beam3").split(",")
with torch.no_grad():
    model.eval()
    res["encode_ms"] = round(timed(lambda: decode.encode_for_generation(model, batch, ["tva"])) * 1e3, 1)
    for name, beam, mode in (("greedy", 1, None), ("beam3", 3, None), ("sample", 1, "sample")):
        if name not in MODES:
            continue
        t = timed(lambda: decode.generate_cap(model, batch, ["tva"], beam_size=beam, max_generation_len=L, mode=mode), reps=2)
        res[name] = {"seconds": round(t, 3), "captions_per_s": round(B / t, 1), "tokens_per_s": round(B * L / t, 1),
                     "ms_per_decoding_step": round((t * 1e3 - res["encode_ms"]) / L, 2)}

SAMPLED = (("filters_off", {}), ("top_k_50", {"top_k": 50}), ("top_p_0.9", {"top_p": 0.9}),
           ("t0.7_k50_p0.9", {"temperature": 0.7, "top_k": 50, "top_p": 0.9}))


def sampler_launch_us(R, V, inv, k, p, filtered):
    """one sampler launch on R rows of V logits: device events around 20 launches, the median of 15 such groups"""
    from valor_amd import kernels as K
    logits = torch.zeros((R, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :V]
    logits.copy_(torch.randn((R, V), generator=torch.Generator().manual_seed(V)) * 2)
    unf = torch.ones(R, dtype=torch.bool, device=dev)
    tok = torch.empty(R, dtype=torch.int64, device=dev)
    sents = torch.empty((R, 1), dtype=torch.int64, device=dev)
    lp = torch.empty((R, 1), dtype=torch.float32, device=dev)
    kept = torch.empty(R, dtype=torch.int32, device=dev)

    def launch(i):
        if filtered:                                        # (kept given: the filtered kernel runs even with every filter off)
            K.sample_tokens_filtered(logits, 1, i * R * V, 0, unf, tok, sents[:, 0], lp[:, 0], inv, k, p, kept)
        else:
            K.sample_tokens(logits, 1, i * R * V, 0, unf, tok, sents[:, 0], lp[:, 0])
    logits[:, 0] = -float("inf")                            # column 0 is the end token here: never drawn, no row finishes
    for i in range(10):
        launch(i)
    times = []
    for _ in range(15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(20):
            launch(i)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / 20)
    assert bool(unf.all())
    return round(sorted(times)[len(times) // 2], 2)


if "sampled" in MODES:
    with torch.no_grad():
        model.eval()
        out = res["sampled"] = {}
        for name, kw in SAMPLED:
            t = timed(lambda: decode.generate_cap(model, batch, ["tva"], max_generation_len=L, mode="sample", seed=1, **kw), reps=3)
            out[name] = {"seconds": round(t, 4), "captions_per_s": round(B / t, 1),
                         "ms_per_decoding_step": round((t * 1e3 - res["encode_ms"]) / L, 3)}
        n = 4
        small = {k: (v[:B // n] if torch.is_tensor(v) else v) for k, v in batch.items()}
        t = timed(lambda: decode.generate_cap(model, small, ["tva"], max_generation_len=L, mode="sample", seed=1, temperature=0.7, top_k=50,
                                              top_p=0.9, num_return_sequences=n), reps=3)
        out[f"t0.7_k50_p0.9_x{n}_at_{B // n}_clips"] = {"seconds": round(t, 4), "captions_per_s": round(B // n * n / t, 1)}
        kern = res["sampler_launch_us"] = {}
        for V in (30522, 49408):
            kern[f"V{V}"] = {"valor_sample_tokens": sampler_launch_us(B, V, 1.0, 0, 1.0, False),
                             "filtered_all_off": sampler_launch_us(B, V, 1.0, 0, 1.0, True),
                             "filtered_top_k_50": sampler_launch_us(B, V, 1.0, 50, 1.0, True),
                             "filtered_top_p_0.9": sampler_launch_us(B, V, 1.0, 0, 0.9, True),
                             "filtered_t0.7_k50_p0.9": sampler_launch_us(B, V, 1 / 0.7, 50, 0.9, True)}

if "scst" in MODES:
    import numpy as np
    from valor_amd import scst
    rng = np.random.default_rng(0)
    batch["ids"] = [f"clip{i}" for i in range(B)]
    model.scorer = scst.CaptionScorer({i: [rng.integers(1000, 3000, size=int(rng.integers(6, 15))).tolist() for _ in range(20)]
                                       for i in batch["ids"]})
    SCORER = os.environ.get("GEN_SCORER", "host")
    if SCORER not in ("host", "device"):
        raise SystemExit(f"GEN_SCORER={SCORER}: host or device")
    on_device = SCORER == "device"
    if on_device:
        model.scorer = model.scorer.to_device(dev, vocab=spec.vocab)
    res["scorer"] = SCORER
    model.max_generation_len = L
    groups = ["tva", "tv"]

    def split():
        t = {}
        sync = torch.cuda.synchronize
        sync(); t0 = time.perf_counter()
        greedy = model.scst_baseline(batch, groups, device=on_device)
        sync(); t["greedy_ms"] = time.perf_counter() - t0; t0 = time.perf_counter()
        vo, ao = model.scst_encode(batch, groups)
        samples = model.scst_sample(vo, ao, groups)
        sync(); t["encode_and_sample_ms"] = time.perf_counter() - t0; t0 = time.perf_counter()
        if on_device:
            rewards = dict(zip(groups, model.scorer.advantages(batch["ids"], [samples[g][0] for g in groups], [greedy[g] for g in groups],
                                                               model.eos_token, vocab=spec.vocab)))
            sync()
        else:
            rewards = {g: model.scorer(batch["ids"], scst.hypotheses(samples[g][0].cpu(), model.eos_token))
                       - model.scorer(batch["ids"], scst.hypotheses(greedy[g], model.eos_token)) for g in groups}
        t["score_ms"] = time.perf_counter() - t0; t0 = time.perf_counter()
        out = model.scst_loss(vo, ao, {g: samples[g][0] for g in groups}, rewards)
        sum(out.values()).backward()
        sync(); t["loss_pass_fwd_bwd_ms"] = time.perf_counter() - t0
        model.zero_grad()
        return t

    model.train()
    split()
    runs = [split() for _ in range(3)]
    res["scst_step"] = {k: round(1e3 * sum(r[k] for r in runs) / len(runs), 3 if k == "score_ms" else 1) for k in runs[0]}
    hyps = [rng.integers(1000, 3000, size=L).tolist() for _ in range(B)]
    if on_device:
        hyps = torch.tensor(hyps, dtype=torch.int64, device=dev)
        call = lambda: model.scorer.score(batch["ids"], hyps, model.eos_token)
        call()
    else:
        call = lambda: model.scorer(batch["ids"], hyps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    res["scorer_ms_per_call"] = round((time.perf_counter() - t0) / 5 * 1e3, 3 if on_device else 2)
print(json.dumps(res, indent=1))
json.dump(res, open(sys.argv[1], "w"), indent=1)
