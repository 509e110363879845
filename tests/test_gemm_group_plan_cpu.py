"""Host side of the grouped weight-gradient launch: the slice plan (valor_gemm_group_plan, csrc/gemm_group_plan.h) for the layers of the
benchmarked step and for the groups of tests/test_gemm_group_gpu.py, the refusals of valor_gemm_group_problem / valor_gemm_group before
any launch, and the exactness conditions of the GPU test's operands (checked here so that a case that stops being exact fails without
a GPU)."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gemm_group_gpu as G  # noqa: E402


def _plan(shapes):
    from valor_amd import lib
    so = lib.load()
    n = len(shapes)
    arr = (ctypes.c_int * (4 * n))(*[v for s in shapes for v in s])
    slices, ksteps, info = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * 4)()
    rc = so.valor_gemm_group_plan(ctypes.cast(arr, ctypes.c_void_p), n, ctypes.cast(slices, ctypes.c_void_p), ctypes.cast(ksteps, ctypes.c_void_p),
                                  ctypes.cast(info, ctypes.c_void_p))
    return rc, list(slices), list(ksteps), list(info)


def test_plan_of_the_step_layers():
    dec = [(768, 3072, 8832, 0), (3072, 768, 8832, 1), (768, 768, 8832, 0), (768, 768, 8832, 1), (768, 768, 8832, 0), (2304, 768, 8832, 1)]
    rc, slices, ksteps, info = _plan(dec)
    assert rc == 0 and slices == [2] * 6 and ksteps == [69] * 6 and info[:3] == [252, 69, 1]          # 126 tiles x 2, four-wave loop
    ast = [(768, 3072, 16512, 0), (3072, 768, 16512, 1), (768, 768, 16512, 0), (2304, 768, 16512, 1)]
    rc, slices, ksteps, info = _plan(ast)
    assert rc == 0 and slices == [2] * 4 and ksteps == [129] * 4 and info[:3] == [216, 129, 1]
    rc, slices, ksteps, info = _plan(dec + dec[:2])                  # more than half a round of tiles: unsplit, no workspace
    assert rc == 0 and slices == [1] * 8 and info[0] == 198 and info[3] == 0
    rc, slices, ksteps, info = _plan([(768, 768, 8832, 0)])          # alone: the rule of a single launch, 9 tiles x 23 slices of 6
    assert rc == 0 and slices == [23] and ksteps == [6] and info[:3] == [207, 6, 0]


def test_plan_of_the_test_groups():
    for name, idx in G.GROUPS.items():
        shapes = [(G.PROBLEMS[i][0], G.PROBLEMS[i][1], G.PROBLEMS[i][2], int(bool(G.PROBLEMS[i][3]))) for i in idx[:8]]
        rc, slices, ksteps, info = _plan(shapes)
        assert rc == 0 and info[0] <= 256 and min(ksteps) >= 6, (name, slices, ksteps, info)
        for (M, N, K, _), s, ks in zip(shapes, slices, ksteps):
            assert s > 1 and (s - 1) * ks < K // 64 <= s * ks, (name, M, N, K, s, ks)            # split, K covered, no empty slice
        if name == "mixedK":            # two contraction lengths: slices in proportion, K-tiles per workgroup within one of each other
            per = [-(-(K // 64) // s) for (_, _, K, _), s in zip(shapes, slices)]
            assert len(set(slices)) > 1 and max(per) - min(per) <= 1, (slices, per)


def test_refusals_before_any_launch():
    from valor_amd import lib
    so = lib.load()
    blob = (ctypes.c_char * 512)()
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = (lib.DT_BF16, 768, 768, 8832, p, 768, p, 768, p, 768, 1.0, 1, None, 0)
    assert so.valor_gemm_group_problem(ctypes.addressof(blob), *ok) == 0
    for bad in ((lib.DT_F32,) + ok[1:],                                     # fp32
                ok[:3] + (8832 + 32,) + ok[4:],                             # K % 64
                ok[:1] + (128,) + ok[2:],                                   # M < 256: not family 3
                ok[:3] + (2048,) + ok[4:],                                  # K < 4096: not family 3
                (lib.DT_BF16, 3072, 768, 100864) + ok[4:],                  # the ViT fc1 wgrad: 225 K-tiles per workgroup alone, keeps its launch
                ok[:11] + (0,) + ok[12:],                                   # no C +=
                ok[:5] + (772,) + ok[6:],                                   # lda % 8
                ok[:4] + (p + 2,) + ok[5:]):                                # misaligned A
        assert so.valor_gemm_group_problem(ctypes.addressof(blob) + 256, *bad) == -1, bad
    assert so.valor_gemm_group(None, lib.DT_BF16, ctypes.addressof(blob), 0, None, 0) == 0             # n = 0: no-op
    assert so.valor_gemm_group(None, lib.DT_BF16, ctypes.addressof(blob), 9, None, 0) == -1
    assert so.valor_gemm_group(None, lib.DT_BF16, ctypes.addressof(blob), 2, None, 0) == -1            # the second blob describes nothing
    assert so.valor_gemm_group(None, lib.DT_BF16, ctypes.addressof(blob), 1, None, 0) == -1            # splits, and has no workspace
    assert so.valor_gemm_group(None, lib.DT_BF16, ctypes.addressof(blob), 1, 256, 1 << 20) == -1       # ... or too small a one


def test_gpu_test_operands_are_exact():
    for i in range(len(G.PROBLEMS)):
        case, ref = G.exact_problem(i)
        assert float(ref["C"].abs().max()) <= 256.0
    p, q = G.exact_problem(0)[1], G.exact_problem(8)[1]
    assert float((p["C"] + q["C"] - q["C0"]).abs().max()) <= 256.0          # the repeated-target test's sum of two products
