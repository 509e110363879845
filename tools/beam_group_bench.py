"""Cost and effect of diverse (group) beam search at the generation geometry (tools/beam_pool_bench.py's: B clips of 8 frames + 2 audio
slices, group 'tva', max_generation_len L, random weights -- they hardly ever emit [SEP], so every row runs the full length): the pool
search at beam 4 and 8 against the group search at (beam, groups) = (4, 2), (4, 4), (8, 2), (8, 4), n = beam hypotheses returned, all
runs alternating in one process, each measured twice. Per configuration:
  captions/s of generate_cap(beam_search='pool'[, num_beam_groups, diversity_penalty]);
  the step launch alone (valor_beam_pool_step / valor_beam_group_step on B samples x beam rows of random logits, device events over a
  burst of launches) at the model's vocabulary, and at a vocabulary of 64 words where the scan of the rows is negligible: what is left
  is the arg-max rounds, the barriers and the one-thread walks, so the difference of the two is the scan;
  what the feature is for: the number of distinct sequences among the n returned per clip, and the share of distinct bigrams among all
  bigrams of a clip's n captions (each cut at its [SEP]).
usage: python tools/beam_group_bench.py out.json [batch] [max_len] [diversity_penalty]   (profiles/beam_group_bench.json)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from valor_amd import decode, synth  # noqa: E402

CONFIGS = [(4, 1), (8, 1), (4, 2), (4, 4), (8, 2), (8, 4)]               # (beam, groups); one group: the pool search


def name(K, G):
    return f"pool_beam{K}" if G == 1 else f"group_beam{K}_groups{G}"


def diversity(seqs, n, eos):
    """seqs: [clips * n, L] rows of token ids, clip-major (a tensor or lists), every row cut at its first eos -> (mean number of distinct
    sequences among a clip's n, mean over the clips of distinct bigrams / all bigrams of the clip's n captions; a clip without a bigram
    counts 0)"""
    rows = seqs.tolist() if torch.is_tensor(seqs) else [list(r) for r in seqs]
    distinct, share = [], []
    for i in range(len(rows) // n):
        cut = [r[:r.index(eos)] if eos in r else r for r in rows[i * n:(i + 1) * n]]
        distinct.append(len({tuple(r) for r in cut}))
        grams = [(r[j], r[j + 1]) for r in cut for j in range(len(r) - 1)]
        share.append(len(set(grams)) / len(grams) if grams else 0.0)
    return round(sum(distinct) / len(distinct), 3), round(sum(share) / len(share), 4)


def summarise(res, B, runs, burst, stats):
    """the result line: runs {(K, G): [seconds of a generate_cap call]}, burst {(K, G): {'vocab' | 'vocab64': [us per launch]}},
    stats {(K, G): diversity(...)} -> res with one entry per configuration, and for the group searches the ratios to the pool search of
    the same beam in the same run (captions/s: > 1 is faster; step launch: > 1 is dearer)"""
    for (K, G), ts in runs.items():
        res[name(K, G)] = {"seconds": [round(t, 4) for t in ts], "captions_per_s": [round(B / t, 1) for t in ts],
                           "step_launch_us": [round(x, 1) for x in burst[K, G]["vocab"]],
                           "step_launch_us_vocab64": [round(x, 1) for x in burst[K, G]["vocab64"]],
                           "n": K, "distinct_sequences_of_n": stats[K, G][0], "distinct_bigram_share": stats[K, G][1]}
    mean = lambda c, key: sum(res[name(*c)][key]) / len(res[name(*c)][key])
    for K, G in runs:
        if G > 1 and (K, 1) in runs:
            res[name(K, G)]["captions_per_s_vs_pool"] = round(mean((K, G), "captions_per_s") / mean((K, 1), "captions_per_s"), 4)
            res[name(K, G)]["step_launch_vs_pool"] = round(mean((K, G), "step_launch_us") / mean((K, 1), "step_launch_us"), 3)
            res[name(K, G)]["step_launch_vs_pool_vocab64"] = round(mean((K, G), "step_launch_us_vocab64") /
                                                                   mean((K, 1), "step_launch_us_vocab64"), 3)
    return res


def timed(fn, reps=2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def step_burst(dev, B, L, K, G, V, lam, launches=50):
    """microseconds per step launch: a state in the middle of a search (an even step near L / 2, every slot live, empty pools), random
    logits; the launch reads scores / hist [0] and writes [1], the same work every time"""
    g = torch.Generator().manual_seed(K * 10 + G)
    z = torch.randn((K * B, V), generator=g).to(dev)
    lse = decode.row_lse(z)[0]
    eos = decode.EOS if V > decode.EOS else 2
    st = decode.PoolState(B, K, L, 0.0, dev, eos) if G == 1 else decode.GroupPoolState(B, K, G, L, 0.0, dev, eos, diversity_penalty=lam)
    t = L // 2 // 2 * 2
    st.scores[0].copy_(-torch.rand((B, K), generator=g) * 4)
    step = decode.beam_pool_step if G == 1 else decode.beam_group_step
    step(z, lse, st, t, K)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        step(z, lse, st, t, K)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def main(out, B=64, L=30, lam=1.0):
    from valor_amd.model.valor import VALOR
    dev = torch.device("cuda:0")
    spec = synth.base_spec()
    model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device=dev)
    model.load_state_dict(synth.make_state_dict(spec, seed=50), strict=True)
    batch = synth.make_batch(spec, batch=B, frames=8, audio_slices=2, txt_len=32, seed=50)
    batch["video_pixels"] = batch["video_pixels"].to(dev)
    batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
    res = {"batch": B, "frames": 8, "audio_slices": 2, "max_generation_len": L, "group": "tva", "diversity_penalty": lam, "vocab": spec.vocab}
    with torch.no_grad():
        model.eval()
        call = {}
        for K, G in CONFIGS:
            kw = dict(num_beam_groups=G, diversity_penalty=lam) if G > 1 else {}
            call[K, G] = lambda K=K, kw=kw: decode.generate_cap(model, batch, ["tva"], beam_size=K, max_generation_len=L, beam_search="pool",
                                                                num_return_sequences=K, **kw)
        for fn in call.values():                                         # the sessions, their captured steps and every kernel once
            fn()
        runs, outs = {c: [] for c in CONFIGS}, {}
        for _ in range(2):                                               # interleaved: every configuration, and again
            for c in CONFIGS:
                t, outs[c] = timed(call[c])
                runs[c].append(t)
        burst = {c: {"vocab": [], "vocab64": []} for c in CONFIGS}
        for _ in range(2):
            for K, G in CONFIGS:
                burst[K, G]["vocab"].append(step_burst(dev, B, L, K, G, spec.vocab, lam))
                burst[K, G]["vocab64"].append(step_burst(dev, B, L, K, G, 64, lam))
    stats = {(K, G): diversity(outs[K, G]["generated_sequences_t_va"].cpu(), K, decode.EOS) for K, G in CONFIGS}
    summarise(res, B, runs, burst, stats)
    print(json.dumps(res))
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    a = sys.argv
    main(a[1], int(a[2]) if len(a) > 2 else 64, int(a[3]) if len(a) > 3 else 30, float(a[4]) if len(a) > 4 else 1.0)
