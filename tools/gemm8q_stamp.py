"""Per-wave cycle stamps of the four-wave wgrad kernel (csrc/gemm8q.hip built -DQ8_STAMP by tools/build_stamp_lib.sh q8, loaded through
VALOR_HIP_LIB): where one K-tile goes -- MFMA issue and the lgkmcnt wait of every slot, the vmcnt wait and the barrier of the two barrier slots --,
cycles per K-tile over the whole loop and the in-kernel clock (s_memtime over s_memrealtime around the loop), after
WARM_S seconds of back-to-back launches on random data. Medians over all waves of all workgroups with more than 8 K-tiles.
The lgkmcnt figures include the return of the s_memtime in front of the wait: compare builds (tools/build_stamp_lib.sh q8 ablate), not
absolute waits. usage: VALOR_HIP_LIB=valor_amd/libvalor_hip_q8stamp.so python tools/gemm8q_stamp.py out.json"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from valor_amd import kernels as K, lib  # noqa: E402

M, MKV, W, I = 100864, 117376, 768, 3072
SHAPES = [("vit_fc1_wgrad", I, W, M), ("vit_qkv_wgrad", 3 * W, W, M), ("kv_wgrad", 2 * W, W, MKV)]
WARM_S = 2.5
STAMP_TILE = 5


def segments():
    """(name, kind, first stamp, last stamp) of every interval inside the stamped K-tile, in program order (indices into the row's [16..])"""
    out = []
    for s in range(8):
        out.append((f"s{s} mfma", "mfma", 2 * s, 2 * s + 1))
        if s in (3, 7):
            v = 17 + 2 * (s >> 1)
            out += [(f"s{s} lgkmcnt", "lgkm", 2 * s + 1, v), (f"s{s} vmcnt", "vmcnt", v, v + 1), (f"s{s} barrier", "barrier", v + 1, 2 * s + 2)]
        else:
            out.append((f"s{s} lgkmcnt", "lgkm", 2 * s + 1, 2 * s + 2))
    return out, 16


def main():
    dev = torch.device("cuda", 0)
    so = lib.load()
    assert hasattr(so, "valor_gemm8q_read_stamps"), "not a -DQ8_STAMP library (tools/build_stamp_lib.sh q8; VALOR_HIP_LIB)"
    so.valor_gemm8q_read_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    res = {"lib": os.environ.get("VALOR_HIP_LIB", "in-tree"), "warmup_s": WARM_S, "stamped_k_tile": STAMP_TILE,
           "unit": "shader cycles (s_memtime), medians over waves; stamps cost cycles themselves: compare builds, not with the shipped kernel"}
    so.valor_gemm_set_policy(12, 1)
    for name, m, n, k in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(1)
        A = torch.randn((k, m), generator=g).to(torch.bfloat16).to(dev)
        B = (0.05 * torch.randn((k, n), generator=g)).to(torch.bfloat16).to(dev)
        out = torch.zeros((m, n), dtype=torch.bfloat16, device=dev)
        rs = torch.zeros((m,), dtype=torch.bfloat16, device=dev)
        fn = lambda: K.gemm(A, B, trans_a=True, trans_b=True, out=out, accumulate=True, rowsum_out=rs, rowsum_accumulate=True)
        assert so.valor_gemm_wave128_for(lib.DT_BF16, 1, 1, m, n, k, 0) == 1
        t0 = time.time()
        while time.time() - t0 < WARM_S:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        raw = np.zeros((1024, 4, 64), dtype=np.uint64)
        assert so.valor_gemm8q_read_stamps(raw.ctypes.data, raw.nbytes) == 0
        raw = raw.astype(np.int64)
        nt = raw[:, :, 10]
        ok = (raw[:, :, 0] > 0) & (nt > 8) & (raw[:, :, 11] == 1)
        st, hs = raw[ok][:, :8].astype(np.float64), raw[ok][:, 16:48].astype(np.float64)
        med = lambda x: float(np.median(x))
        loop = st[:, 2] - st[:, 1]
        row = {"MNK": [m, n, k], "waves": int(ok.sum()), "k_tiles_median": med(nt[ok]),
               "launch_us_with_stamps": round(e0.elapsed_time(e1) / 5 * 1e3, 1),
               "cycles_per_k_tile": med(loop / nt[ok]), "clock_GHz": med(loop / (st[:, 7] - st[:, 6]) * 0.1),
               "prologue": med(st[:, 1] - st[:, 0]), "k_loop": med(loop), "drain_sync": med(st[:, 3] - st[:, 2]),
               "epilogue_pass0": med(st[:, 4] - st[:, 3]), "epilogue_pass1": med(st[:, 5] - st[:, 4])}
        segs, last = segments()
        row["stamped_tile_total"] = med(hs[:, last] - hs[:, 0])
        row["segments"] = {nm: med(hs[:, b] - hs[:, a]) for nm, _, a, b in segs}
        for kind in ("mfma", "lgkm", "vmcnt", "barrier"):
            row["sum_" + kind] = med(sum(hs[:, b] - hs[:, a] for _, kd, a, b in segs if kd == kind))
        res[name] = row
        print(name, json.dumps(row), flush=True)
    so.valor_gemm_set_policy(12, 1000)
    json.dump(res, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
