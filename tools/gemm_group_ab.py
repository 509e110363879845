"""A/B of a layer's weight gradients as one grouped split-K launch (valor_gemm_group, VALOR_GROUP_WGRAD) against today's launches: the
six products of a decoder layer (8832 tokens) and the four of an AST layer (16512 tokens), each  C += dY^T . X  into its own gradient
slot with the bias gradient as fused row sums where ops._wgrad_bgrad fuses it. old = one deferred split-K launch per product + ONE grouped
reduction (6 + 1 / 4 + 1 launches), new = ONE grouped launch + ONE grouped reduction (1 + 1). Same random bf16 operands, interleaved
rounds old / new in one process, HIP events around `reps` layers back to back, every round's time; the grouped launch is also timed
pinned to either kernel (policy key 12 = 0: eight-wave pipelined loop, 1: four-wave slot loop) -- the threshold question of DESIGN.md 8.
usage: python tools/gemm_group_ab.py out.json [rounds]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from valor_amd import kernels as K, lib  # noqa: E402

W, I = 768, 3072
WARM_S = 2.0
# (M, N, fused row sums) in the order the backward pass issues them: fc2, fc1, [cross out, cross query,] attention out, qkv
LAYERS = {"decoder_layer": (8832, [(W, I, False), (I, W, True), (W, W, False), (W, W, True), (W, W, False), (3 * W, W, True)]),
          "ast_layer": (16512, [(W, I, False), (I, W, True), (W, W, False), (3 * W, W, True)])}


def timeit(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    dev = torch.device("cuda", 0)
    so = lib.load()
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    res = {"rounds": rounds, "reps_per_round": 5, "warmup": f"all variants alternating for {WARM_S} s per layer",
           "unit": "us per layer (all its wgrads and their reduction), HIP events"}
    for name, (tokens, shapes) in LAYERS.items():
        g = torch.Generator(device="cpu").manual_seed(1)
        prob = []
        for m, n, rs in shapes:
            a = torch.randn((tokens, m), generator=g).to(torch.bfloat16).to(dev)
            b = (0.05 * torch.randn((tokens, n), generator=g)).to(torch.bfloat16).to(dev)
            prob.append((a, b, torch.zeros((m, n), dtype=torch.bfloat16, device=dev), torch.zeros((m,), dtype=torch.bfloat16, device=dev) if rs else None))

        def layer():
            with K.ReduceQueue.batch():
                for a, b, c, r in prob:
                    K.gemm(a, b, trans_a=True, trans_b=True, out=c, accumulate=True, rowsum_out=r, rowsum_accumulate=True, defer_done=lambda: None)

        variants = {"old": (False, 1000), "new": (True, 1000), "new_eight_wave": (True, 0), "new_four_wave": (True, 1)}

        def run(v, reps):
            K.ReduceQueue.group_wgrad, key12 = variants[v]
            if v != "old":
                so.valor_gemm_set_policy(12, key12)
            t = timeit(layer, reps)
            so.valor_gemm_set_policy(12, 1000)
            return t
        outs = {}
        for v in variants:
            for _, _, c, r in prob:
                c.zero_()
                if r is not None:
                    r.zero_()
            run(v, 1)
            outs[v] = [c.clone() for _, _, c, _ in prob] + [r.clone() for _, _, _, r in prob if r is not None]
        t_warm = time.time()
        while time.time() - t_warm < WARM_S:
            for v in variants:
                run(v, 5)
        t = {v: [] for v in variants}
        for _ in range(rounds):
            for v in variants:
                t[v].append(run(v, 5))
        K.ReduceQueue.group_wgrad = False
        fl = sum(2.0 * m * n * tokens for m, n, _ in shapes)
        row = {"tokens": tokens, "shapes": [[m, n] for m, n, _ in shapes]}
        for v, ts in t.items():
            row[v + "_us"] = [round(x, 1) for x in ts]
            row[v + "_TF"] = round(fl / sorted(ts)[rounds // 2] / 1e6, 1)
        row["new_faster_in_every_round"] = bool(all(n < o for n, o in zip(t["new"], t["old"])))
        row["new_slowest_beats_old_fastest"] = bool(max(t["new"]) < min(t["old"]))
        row["median_old_over_new"] = round(sorted(t["old"])[rounds // 2] / sorted(t["new"])[rounds // 2], 4)
        # the two kernels of the grouped launch give the same bits; against the old launches the partial sums are rounded differently
        row["new_kernels_bit_identical"] = all(torch.equal(x, y) for x, y in zip(outs["new_eight_wave"], outs["new_four_wave"]))
        row["max_abs_diff_new_vs_old"] = max(float((x.float() - y.float()).abs().max()) for x, y in zip(outs["new"], outs["old"]))
        res[name] = row
        print(name, row, flush=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
