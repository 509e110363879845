"""What closed answer sets cost, on the bench model (base widths, bf16) at 64 clips of 8 frames + 2 audio slices, one question per clip,
group 'tva', V = 30522:
  * one valor_trie_constrain launch on the step's padded logits at 64 and 192 rows (192 = three beam-major beams of 64 samples), for two
    sets -- four per-sample choices of 1..4 tokens, and a synthetic shared set of 3129 answers of 1..4 tokens (its root has a couple of
    thousand children: the LDS-staged search at its largest) -- at t = 0 (the root) and t = 2, between device events (20 launches per
    event pair, the median of 15 pairs); valor_logits_constrain at the same rows is timed beside it, the way tools/gen_constraints_bench.py
    does (profiles/gen_constraints.json), as the comparison point;
  * decode.generate_qa answers/s, greedy and beam-3, unconstrained against constrained (both sets), alternating in ONE process on kept
    sessions; a setting's figure is the median of its runs. Random weights never emit [SEP], so the unconstrained rows run the full
    max_generation_len while a constrained row ends with its answer: the constrained loops stop early where their end test allows;
  * decode.score_candidates at 64 questions x 5 choices of up to 10 tokens (320 decoder rows, one chunk).
usage: python tools/answer_set_bench.py [out.json] [batch] [max_len] [rounds]      (default profiles/answer_set_bench.json 64 10 5)"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from valor_amd import decode, kernels as K, synth  # noqa: E402
from valor_amd.model.valor import VALOR  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "answer_set_bench.json")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
L = int(sys.argv[3]) if len(sys.argv) > 3 else 10
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
V = 30522
dev = torch.device("cuda:0")
spec = synth.base_spec()
model = VALOR({"dropout": 0.1, "max_generation_len": L}, spec=spec, dtype=torch.bfloat16, device=dev)
model.load_state_dict(synth.make_state_dict(spec, seed=50), strict=True)
batch = synth.make_batch(spec, batch=B, frames=8, audio_slices=2, txt_len=32, seed=50, questions=True)
batch["video_pixels"] = batch["video_pixels"].to(dev)
batch["audio_spectrograms"] = batch["audio_spectrograms"].to(dev)
prompt = model.qa_prompt(batch["question_tokens"]["bert_tokens"].cpu())
res = {"batch": B, "frames": 8, "audio_slices": 2, "max_generation_len": L, "group": "tva", "rounds": ROUNDS, "vocab": V}


def answers(n, lo, hi, g):
    """n distinct answers of lo..hi tokens; ids in [1000, V): no special token"""
    seen, out = set(), []
    while len(out) < n:
        c = tuple(torch.randint(1000, V, (int(torch.randint(lo, hi + 1, (1,), generator=g)),), generator=g).tolist())
        if c not in seen:
            seen.add(c)
            out.append(list(c))
    return out


g = torch.Generator().manual_seed(3129)
first = torch.randint(1000, V, (1800,), generator=g).tolist()                   # the shared set's answers start from 1800 draws of first tokens
shared_list = [[first[int(torch.randint(0, 1800, (1,), generator=g))]] + c[1:] for c in answers(3129, 1, 4, g)]
shared = decode.AnswerSet(shared_list, vocab=V)
four = decode.AnswerSet([answers(4, 1, 4, g) for _ in range(B)], per_sample=True, vocab=V)
five = decode.AnswerSet([answers(5, 1, 10, g) for _ in range(B)], per_sample=True, vocab=V)
res["sets"] = {"shared_3129": {"answers": shared.counts[0], "nodes": shared.n_nodes, "root_children": int(shared.child_ptr[1])},
               "four_per_sample": {"answers": 4, "nodes": four.n_nodes}}


def seconds(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def median(xs):
    return sorted(xs)[len(xs) // 2]


def event_us(go):
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


def launch_us(aset, R, t):
    """rows beam-major over words kept as [B, beam, L]; every row's history follows one of its sample's answers"""
    beam = R // B
    logits = torch.zeros((R, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :V]
    logits.copy_(torch.randn((R, V), generator=torch.Generator().manual_seed(R)) * 2)
    words = torch.full((B, beam, L), decode.EOS, dtype=torch.long)
    for s in range(B):
        for k in range(beam):
            c = aset.candidates[s % aset.n_roots][(s + k) % aset.counts[s % aset.n_roots]]
            words[s, k, :len(c)] = torch.tensor(c)
    words, trie = words.to(dev), aset.device(dev)
    return event_us(lambda: K.trie_constrain(logits, words, t, decode.EOS, trie, None, B, beam * L, L))


def constrain_us(R, t):
    logits = torch.zeros((R, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)[:, :V]
    hist = torch.randint(1000, 1000 + 12, (R, t + 1), generator=torch.Generator().manual_seed(t)).to(dev)
    c = decode.Constraints(no_repeat_ngram_size=3, repetition_penalty=1.2, min_length=5)
    return event_us(lambda: K.logits_constrain(logits, hist, t, decode.EOS, c.penalty, c.inv_penalty, c.no_repeat_ngram_size, c.min_length))


with torch.no_grad():
    model.eval()
    res["trie_launch_us"] = {f"{name}_R{R}_t{t}": launch_us(a, R, t) for name, a in (("four_per_sample", four), ("shared_3129", shared))
                             for R in (B, 3 * B) for t in (0, 2)}
    res["logits_constrain_launch_us"] = {f"R{R}_t{L - 1}": constrain_us(R, L - 1) for R in (B, 3 * B)}
    enc = [seconds(lambda: decode.encode_for_generation(model, batch, ["tva"])) for _ in range(4)]
    res["encode_ms"] = round(median(enc[1:]) * 1e3, 1)
    for name, beam in (("greedy", 1), ("beam3", 3)):
        gen = lambda a: (lambda: decode.generate_qa(model, batch, ["tva"], prompt, beam_size=beam, candidates=a))
        run = {"unconstrained": gen(None), "four_per_sample": gen(four), "shared_3129": gen(shared)}
        for k in run:                                            # first runs: the session, its eager step and the capture
            run[k]()
        times = {k: [] for k in run}
        for _ in range(ROUNDS):
            for k in run:
                times[k].append(seconds(run[k]))
        out = res[name] = {}
        for k in run:
            t = median(times[k])
            out[k] = {"seconds": round(t, 4), "answers_per_s": round(B / t, 1), "runs_s": [round(x, 4) for x in times[k]]}
        for k in ("four_per_sample", "shared_3129"):
            out[k + "_over_unconstrained"] = round(median(times[k]) / median(times["unconstrained"]), 4)
    score = lambda: decode.score_candidates(model, batch, ["tva"], five, prompt_cpu=prompt)
    score()
    ts = [seconds(score) for _ in range(ROUNDS)]
    res["score_candidates"] = {"choices": 5, "max_tokens": five.max_len, "rows": 5 * B, "seconds": round(median(ts), 4),
                               "questions_per_s": round(B / median(ts), 1), "runs_s": [round(x, 4) for x in ts]}
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(res, open(OUT, "w"), indent=1)
