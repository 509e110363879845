"""A/B of family 3's launches on four waves of 128 x 128 outputs (csrc/gemm8q.hip, policy key 12) against the eight-wave kernel of
gemm8.hip at the step's long-K shapes. Same random bf16 operands, interleaved rounds old / new in one process, HIP events around `reps`
back-to-back calls (a split-K product includes its reduction launch, the same one on both sides), every round's time and TF/s.
A shape whose layout gemm8q.hip does not have (valor_gemm_wave128_for == 0 under key 12 = 1) is listed as such and not timed.
usage: python tools/gemm_wave128_ab.py out.json [rounds] [gate]        ("gate": only the ViT fc1 wgrad, the go / no-go problem)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from valor_amd import kernels as K, lib  # noqa: E402

M, MKV, W, I = 100864, 117376, 768, 3072
WARM_S = 3.0
# (name, layout, M, N, K): layout tt = wgrad (dY^T . X), nn = forward, nt = dgrad
SHAPES = [("vit_fc1_wgrad", "tt", I, W, M), ("vit_fc2_wgrad", "tt", W, I, M), ("vit_qkv_wgrad", "tt", 3 * W, W, M), ("vit_proj_wgrad", "tt", W, W, M),
          ("kv_wgrad", "tt", 2 * W, W, MKV), ("ast_fc1_wgrad", "tt", I, W, 16512), ("dec_fc1_wgrad", "tt", I, W, 8832),
          ("vit_fc2_fwd", "nn", M, W, I), ("vit_fc1_dgrad", "nt", M, W, I), ("vit_qkv_dgrad", "nt", M, W, 3 * W), ("kv_dgrad", "nt", MKV, W, 2 * W)]


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
    gate = len(sys.argv) > 3 and sys.argv[3] == "gate"
    res = {"rounds": rounds, "reps_per_round": 5, "warmup": f"both kernels alternating for {WARM_S} s per shape",
           "unit": "us per call, HIP events; split-K products include their reduction launch"}
    for name, lay, m, n, k in (SHAPES[:1] if gate else SHAPES):
        ta, tb = (1, 1) if lay == "tt" else (0, 0) if lay == "nn" else (0, 1)
        so.valor_gemm_set_policy(12, 1)
        built = so.valor_gemm_wave128_for(lib.DT_BF16, ta, tb, m, n, k, 0)
        so.valor_gemm_set_policy(12, 0)
        row = {"layout": lay, "MNK": [m, n, k], "family": so.valor_gemm_kernel_for(lib.DT_BF16, ta, tb, m, n, k, 0), "wave128_built": built}
        if not built:
            res[name] = row
            print(name, row, flush=True)
            continue
        g = torch.Generator(device="cpu").manual_seed(1)
        A = torch.randn((k, m) if ta else (m, k), generator=g).to(torch.bfloat16).to(dev)
        B = (0.05 * torch.randn((k, n) if tb else (n, k), generator=g)).to(torch.bfloat16).to(dev)
        out = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)
        rs = torch.zeros((m,), dtype=torch.bfloat16, device=dev) if lay == "tt" else None
        if lay == "tt":        # as ops._wgrad_bgrad launches it: C += into the gradient slot, bias gradient as fused row sums
            fn = lambda: K.gemm(A, B, trans_a=True, trans_b=True, out=out, accumulate=True, rowsum_out=rs, rowsum_accumulate=True)
        else:
            fn = lambda: K.gemm(A, B, trans_b=bool(tb), out=out)
        outs = {}
        for key, v in (("old", 0), ("new", 1)):       # same bits first
            so.valor_gemm_set_policy(12, v)
            out.zero_()
            if rs is not None:
                rs.zero_()
            fn()
            outs[key] = (out.clone(), None if rs is None else rs.clone())
        t_warm = time.time()                           # both kernels until the clocks have settled: a cold device drifts by 10-25 % over its first second
        while time.time() - t_warm < WARM_S:
            for v in (0, 1):
                so.valor_gemm_set_policy(12, v)
                timeit(fn, 10)
        t = {"old": [], "new": []}
        for _ in range(rounds):
            for key, v in (("old", 0), ("new", 1)):
                so.valor_gemm_set_policy(12, v)
                t[key].append(timeit(fn, 5))
        so.valor_gemm_set_policy(12, 1000)
        fl = 2.0 * m * n * k
        for key, v in t.items():
            row[key + "_us"] = [round(x, 1) for x in v]
            row[key + "_TF"] = [round(fl / x / 1e6, 1) for x in v]
        row["old_spread_us"] = round(max(t["old"]) - min(t["old"]), 1)
        row["new_slowest_beats_old_fastest"] = bool(max(t["new"]) < min(t["old"]))
        row["median_new_over_old_speed"] = round(sorted(t["old"])[rounds // 2] / sorted(t["new"])[rounds // 2], 4)
        res[name] = row
        print(name, row, flush=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
