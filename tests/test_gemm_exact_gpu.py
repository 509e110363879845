"""Every GEMM family of valor_gemm (csrc/gemm.hip, gemm8.hip, gemm8q.hip, gemm8n.hip, gemm8w.hip, gemm_skinny.hip) element for element
against an integer reference computed on the host, on inputs for which the result does not depend on the summation order or on how
often it is rounded (tests/gemm_exact.py): tolerance ZERO, every output inside guard rows / guard columns that must keep their canary.
The norm tests of the other GEMM files let a dozen wrong elements, a swapped row pair or a bias shifted on a tail through
(tests/test_gemm_exact_inputs_cpu.py measures how far under their bounds those stay); equality between two kernels that share a K loop
passes two kernels that are wrong the same way. Here each case pins the kernel through the tuning hooks, ASSERTS through
valor_gemm_kernel_for* / valor_gemm_wave128_for that the family it means to test is the one that runs, and restores every hook afterwards.
Reference semantics: nn.Linear and its autograd GEMMs with the fused epilogues of include/valor_hip.h (valor_gemm)."""
import ctypes
import os

import pytest
import torch

import gemm_exact as GE
from gemm_exact import ACT_DERIV, ACT_RELU, Case

pytestmark = pytest.mark.gpu

LAYOUTS = {"NN": (False, False), "NT": (False, True), "TN": (True, False), "TT": (True, True)}
RD = ACT_RELU | ACT_DERIV
# the exact epilogues (alpha = 2 doubles the sums: a smaller budget keeps 2 * sum + 30 inside 256)
EPI = {
    "plain": {},
    "half": dict(alpha=0.5),
    "two_bias": dict(alpha=2.0, bias=True, budget=32),
    "bias": dict(bias=True),
    "relu": dict(bias=True, act=ACT_RELU),
    "relu_nb": dict(act=ACT_RELU),      # (the first 30 bias values are negative: behind them a ReLU of a 16- or 24-column product is all zero)
    "relu_pre": dict(bias=True, act=ACT_RELU, preact=True),
    "relu_dsave": dict(bias=True, act=RD, preact=True),
    "dmul": dict(act=RD, aux="deriv"),
    "drelu": dict(act=ACT_RELU, aux="relu"),
    "acc": dict(acc=True),
    "acc_bias": dict(acc=True, bias=True),
    "f32": dict(out_f32=True),
    "f32_acc_bias": dict(out_f32=True, acc=True, bias=True),
    # fp32 results of DENSE bf16 operands ([-3, 3]: sums of thousands): nothing on the way may pass through bf16
    "f32_dense": dict(out_f32=True, dense=True),
    "f32_dense_acc_bias": dict(out_f32=True, dense=True, acc=True, bias=True),
    "f32_dense_relu_pre": dict(out_f32=True, dense=True, bias=True, act=ACT_RELU, preact=True),
    "rs_f32_dense": dict(rowsum="acc", out_f32=True, dense=True),
    "rs": dict(rowsum="plain"),
    "rs_acc": dict(rowsum="acc", acc=True),
    "rs_f32": dict(rowsum="acc", out_f32=True),
}
GENERAL = ["plain", "half", "two_bias", "relu", "relu_pre", "relu_dsave", "dmul", "drelu", "acc", "f32", "f32_acc_bias"]
ROWSUMS = ["rs", "rs_acc", "rs_f32"]
LD_EXTRA = [8, 4, 3]

# ---- shapes: the smallest that reach each edge. 128x128 families: one tile, one more / fewer than a tile, partly empty last wave /
# 16-row fragment / 8-column chunk, N % 8 == 4, N % 4 != 0, one / two / three K-tiles and seven
S128 = [(128, 128, 64), (129, 136, 128), (70, 136, 192), (304, 264, 448), (100, 260, 64), (257, 130, 128), (8, 8, 8), (384, 328, 192)]
# 256x256 family: M, N >= 256, K >= 128 in whole K-tiles; 328 / 384: a half-empty last tile column
S256 = [(256, 256, 128), (257, 264, 192), (304, 520, 448), (1000, 328, 128), (520, 384, 192), (512, 516, 128), (300, 262, 128)]
# 256x128 family: M >= 256, N >= 128
S256N = [(256, 128, 128), (257, 136, 192), (304, 520, 448), (1000, 328, 128), (700, 384, 192), (512, 132, 128), (300, 262, 192)]
# fp32 products (family 0, dense [-3, 3] operands, alignment unit 4): K-tile 32
SF32 = [(128, 128, 32), (70, 136, 40), (129, 260, 100), (304, 130, 448), (8, 8, 8), (257, 134, 64)]


def _case(name, family, shape, lay, epi, knobs, i=0, **kw):
    ta, tb = LAYOUTS[lay]
    M, N, K = shape
    args = dict(EPI[epi])
    args.update(kw)
    args.setdefault("ld_extra", LD_EXTRA[i % 3])
    return Case(name=f"{name}-{lay}-{M}x{N}x{K}-{epi}-ld{args['ld_extra']}", family=family, M=M, N=N, K=K, ta=ta, tb=tb,
                knobs=tuple(knobs), seed=1 + i % 2, **args)


def _rotate(name, family, shapes, layouts, epis, knob_sets, offset=0, **kw):
    """one case per (layout, epilogue); shapes, leading-dimension paddings and knob sets rotate underneath (coprime strides), so that over the
    table every shape, every padding and every knob value meets every layout and most epilogues without the full product"""
    out, i = [], offset
    for lay in layouts:
        for epi in epis:
            if EPI[epi].get("rowsum") and not LAYOUTS[lay][0]:
                continue
            kn = knob_sets[i % len(knob_sets)]
            out.append(_case(name + "".join(f"-{k}{v}".replace(",", "x") for k, v in kn if k != "variant"), family, shapes[(i * 5 + offset) % len(shapes)], lay,
                             epi, kn, i, **kw))
            i += 1
    return out


def _build_cases():
    C = []
    ALL = list(LAYOUTS)
    # ---- family 0: register-staged 128x128, bf16 (variant 0) and every fp32 product
    C += _rotate("f0", 0, S128, ALL, GENERAL, [(("variant", 0),)])
    C += _rotate("f0", 0, S128, ALL, ["plain", "relu_pre", "acc_bias"], [(("variant", 0),)], offset=5)
    C += _rotate("f32", 0, SF32, ALL, GENERAL[:-2], [()], f32=True)
    C += _rotate("f32", 0, SF32, ALL, ["bias", "acc"], [()], offset=4, f32=True)
    # ---- families 1 / 2: LDS-DMA 128x128, single / double stage; lean (plain, alpha, bias, C +=, fp32) and fused epilogue instantiations
    for v in (1, 2):
        C += _rotate(f"f{v}", v, S128, ALL, GENERAL, [(("variant", v),)], offset=v)
        C += _rotate(f"f{v}", v, S128, ALL, ["bias", "relu_dsave", "acc"], [(("variant", v),)], offset=4 + v)
    # ---- family 3: 256x256 8-phase, eight waves. Schedules x transposing-read flavours x tile-epilogue modes x raster x store mode
    k3 = [(("variant", 3), ("key12", 0), ("sched", s), ("tr_asm", t), ("fast_epi", f), ("key4", r), ("key5", st))
          for s, t, f, r, st in [(0, 0, 0, 0, 0), (1, 1, 1, 2, 1), (0, 1, 2, 1000, 0), (1, 0, 2, 0, 1), (0, 1, 1, 2, 0), (1, 1, 0, 1000, 1),
                                 (1, 1, 2, 2, 0), (0, 0, 1, 1000, 1), (1, 0, 1, 0, 0), (0, 1, 0, 2, 1), (0, 0, 2, 2, 1)]]
    C += _rotate("f3", 3, S256, ALL, GENERAL + ROWSUMS, k3)
    C += _rotate("f3", 3, S256, ALL, GENERAL + ROWSUMS, k3, offset=4)
    # the tile epilogue needs N % 8 == 0 and ldc % 8 == 0: every mode of it on every epilogue it has, on shapes that qualify
    k3f = [(("variant", 3), ("key12", 0), ("sched", s), ("tr_asm", 1), ("fast_epi", f), ("key4", r), ("key5", st))
           for s, f, r, st in [(0, 1, 2, 0), (1, 2, 1000, 1), (1, 1, 0, 1), (0, 2, 2, 0)]]
    C += _rotate("f3tile", 3, [(257, 264, 192), (304, 520, 448), (1000, 328, 128)], ["NN", "NT"],
                 ["plain", "half", "two_bias", "relu", "relu_pre", "relu_dsave", "dmul", "drelu", "acc", "acc_bias"], k3f, ld_extra=8)
    # K = 3200 without split-K: 50 K-tiles per workgroup (the automatic schedule takes the eight-barrier loop above 48, the pipelined one below)
    for i, (lay, epi, sched) in enumerate([("TT", "plain", 1000), ("TT", "rs_acc", 1000), ("TT", "f32", 0), ("TT", "acc", 1), ("NN", "bias", 1000),
                                           ("NT", "dmul", 1000)]):
        C.append(_case(f"f3long-sched{sched}", 3, (304, 264, 3200), lay, epi, (("variant", 3), ("key12", 0), ("sched", sched)), i))
    C.append(_case("f3short-sched1000", 3, (304, 264, 448), "TT", "rs", (("variant", 3), ("key12", 0), ("sched", 1000)), 0))
    # ---- family 3 on four waves (gemm8q.hip): policy key 12 = 1, layout TT
    kq = [(("variant", 3), ("key12", 1), ("sched", s)) for s in (0, 1)]
    C += _rotate("f3q", 3, S256, ["TT"], ["plain", "acc", "f32", "rs", "rs_acc", "rs_f32", "half", "acc_bias"], kq, wave128=True)
    C += _rotate("f3q", 3, S256, ["TT"], ["plain", "acc", "f32", "rs", "rs_acc"], kq, offset=3, wave128=True)
    C.append(_case("f3q-long", 3, (304, 264, 3200), "TT", "rs_acc", kq[0], 1, wave128=True))
    # the measured choice (key 12 = 1000) takes the four-wave kernel above 48 K-tiles per workgroup counted WITH split-K: no shape of this size
    # gets there, the eight-wave kernel keeps it
    C.append(_case("f3q-auto-stays-eight-wave", 3, (304, 264, 3200), "TT", "acc", (("variant", 3), ("key12", 1000)), 2))
    # the other layouts stay on the eight-wave kernel whatever key 12 says
    C.append(_case("f3q-other", 3, (257, 264, 192), "NT", "plain", kq[1], 0))
    # ---- family 4: 256x128, two workgroups per CU (key 8 = 1); schedules, MFMA shape (key 9), 512-thread workgroups (key 10, NN)
    k4 = [(("key8", 1), ("nsched", s), ("key9", m), ("key10", w), ("tr_asm", t), ("fast_epi", f), ("key4", r), ("key5", st))
          for s, m, w, t, f, r, st in [(0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 1, 2, 1), (1, 0, 1, 1, 2, 1000, 0), (0, 1, 0, 1, 2, 0, 1),
                                       (0, 0, 1, 0, 1, 2, 1), (1, 0, 0, 1, 0, 1000, 1), (1, 1, 1, 1, 1, 0, 0), (0, 0, 0, 1, 2, 2, 0),
                                       (1, 0, 1, 0, 0, 2, 0), (0, 1, 0, 0, 1, 1000, 0), (1, 1, 0, 1, 2, 0, 1)]]
    C += _rotate("f4", 4, S256N, ["NN", "NT", "TT"], GENERAL + ROWSUMS, k4)
    C += _rotate("f4", 4, S256N, ["NN", "NT", "TT"], GENERAL + ROWSUMS, k4, offset=5)
    k4f = [(("key8", 1), ("nsched", s), ("key9", m), ("key10", w), ("tr_asm", 1), ("fast_epi", f), ("key4", r), ("key5", st))
           for s, m, w, f, r, st in [(1, 0, 0, 1, 2, 0), (0, 1, 0, 2, 1000, 1), (1, 0, 1, 2, 0, 1), (0, 0, 1, 1, 2, 0), (1, 1, 0, 1, 0, 0)]]
    C += _rotate("f4tile", 4, [(257, 136, 192), (304, 520, 448), (1000, 328, 128)], ["NN", "NT"],
                 ["plain", "half", "two_bias", "relu", "relu_pre", "relu_dsave", "dmul", "drelu", "acc", "acc_bias"], k4f, ld_extra=8)
    C += _rotate("f4tile", 4, [(304, 520, 448), (257, 136, 192)], ["NN"], ["plain", "relu", "relu_pre", "relu_dsave", "dmul", "drelu", "acc"],
                 k4f, offset=2, ld_extra=8)
    # family 4 has no TN kernel: the policy hands that layout to the 128x128 kernel
    C += _rotate("f4-tn", 1, S256N[:4], ["TN"], ["plain", "relu_pre", "acc", "f32"], [(("key8", 1),)])
    # ---- K tails (below 64 and below 8, NaN behind K on a padded leading dimension): the 8-phase families must hand them to family 1
    for j, kn in enumerate([(("variant", 3),), (("key8", 1),), (("variant", 1),), (("variant", 2),), (("variant", 0),)]):
        fam = {0: 0, 2: 2}.get(dict(kn).get("variant", -1), 1)
        for i, (shape, lay, epi) in enumerate([((304, 264, 1001), "NN", "bias"), ((257, 520, 70), "NT", "relu_pre"), ((264, 328, 132), "TT", "acc"),
                                               ((300, 262, 197), "TN", "plain"), ((70, 136, 1001), "NN", "f32")]):
            C.append(_case(f"ktail-{kn[0][0]}{kn[0][1]}", fam, shape, lay, epi, kn, i + j))
    for i, (shape, lay, epi) in enumerate([((70, 136, 1001), "NN", "bias"), ((129, 260, 70), "NT", "relu_pre"), ((130, 132, 133), "TT", "acc"),
                                           ((70, 136, 37), "TN", "plain")]):
        C.append(_case("ktail-f32", 0, shape, lay, epi, (), i, f32=True))
    # ---- split-K. K = 3136 = 49 K-tiles cut into 8 slices of 7: the eighth slice is EMPTY; K = 3200 = 50: the eighth holds one K-tile.
    # bf16 partials (key 1 = 1) and fp32 partials; every epilogue runs in the reduction kernel
    for fam, kn in ((1, (("variant", 1),)), (2, (("variant", 2),)), (3, (("variant", 3), ("key12", 0))), (4, (("key8", 1),))):
        lays = ["NN", "NT", "TT"] if fam == 4 else ALL
        shp = [(304, 520, 3136), (257, 264, 3200)] if fam != 4 else [(304, 520, 3136), (257, 136, 3200)]
        eps = ["plain", "acc", "relu_pre", "f32", "two_bias", "drelu"] + (ROWSUMS if fam >= 3 else [])
        ks = [kn + (("key1", b),) + ((("sched", s), ("nsched", s), ("tr_asm", s)) if fam >= 3 else ()) for b, s in ((1, 0), (0, 1), (1, 1), (0, 0))]
        C += _rotate(f"split-f{fam}", fam, shp, lays, eps, ks, offset=fam, splitk=True, split=True)
    C += _rotate("split-f0", 0, [(304, 264, 3136), (70, 136, 3200)], ALL, ["plain", "acc", "relu_pre", "f32"], [(("variant", 0),)], splitk=True, split=True)
    C += _rotate("split-f32", 0, [(70, 136, 1056), (129, 260, 1001)], ALL, ["plain", "acc_bias", "relu_pre"], [()], splitk=True, split=True, f32=True)
    kq1 = [(("variant", 3), ("key12", 1), ("key1", b)) for b in (1, 0)]
    C += _rotate("split-f3q", 3, [(304, 520, 3136), (257, 264, 3200)], ["TT"], ["plain", "acc", "f32", "rs", "rs_acc", "rs_f32"], kq1,
                 splitk=True, split=True, wave128=True)
    # ---- fp32 results of dense bf16 operands, whole and split (key 1 = 1 asks for bf16 partials: an fp32 result must not get them)
    DENSE = ["f32_dense", "f32_dense_acc_bias", "f32_dense_relu_pre", "rs_f32_dense"]
    for fam, kn, shp, lays in ((0, (("variant", 0),), S128, ALL), (1, (("variant", 1),), S128, ALL), (2, (("variant", 2),), S128, ALL),
                               (3, (("variant", 3), ("key12", 0), ("fast_epi", 2)), S256, ALL), (3, (("variant", 3), ("key12", 1)), S256, ["TT"]),
                               (4, (("key8", 1), ("fast_epi", 2)), S256N, ["NN", "NT", "TT"])):
        eps = DENSE if fam >= 3 else DENSE[:3]
        w = dict(wave128=True) if dict(kn).get("key12") == 1 else {}
        tag = "q" if w else ""
        C += _rotate(f"dense-f{fam}{tag}", fam, [x for x in shp if x[2] >= 16], lays, eps, [kn], offset=fam, **w)
        big = [(304, 520, 3136), (257, 264, 3200)] if fam != 4 else [(304, 520, 3136), (257, 136, 3200)]
        C += _rotate(f"dense-split-f{fam}{tag}", fam, big, lays, eps, [kn + (("key1", 1),)], offset=fam, splitk=True, split=True, **w)
    for i, (shape, tile) in enumerate([((63, 24, 768), "auto"), ((193, 1000, 1024), "4,4"), ((384, 16, 4096), "8,2"), ((2, 1000, 512), "4,1"),
                                       ((65, 24, 3072), "4,2"), ((64, 1000, 768), "8,1")]):
        C.append(_case(f"dense-f5-tile{tile.replace(',', 'x')}", 5, shape, "NN", "f32_dense", (("skinny", 384), ("skinny_tile", tile)), i))
    # a workspace is offered but the product is too short to be cut
    C.append(_case("nosplit-f3", 3, (304, 520, 448), "TT", "rs_acc", (("variant", 3), ("key12", 0)), 0, splitk=True))
    C.append(_case("nosplit-f1", 1, (304, 264, 448), "NN", "relu", (("variant", 1),), 0, splitk=True))
    # ---- a workspace piece of exactly the bytes the slicing needs, cut from a guarded buffer: one per split-K family
    for i, (fam, kn, lay, epi, extra) in enumerate([(0, (("variant", 0),), "NN", "plain", {}), (1, (("variant", 1),), "NT", "acc", {}),
                                                    (2, (("variant", 2),), "TT", "plain", {}), (3, (("variant", 3), ("key12", 0)), "TT", "rs_acc", {}),
                                                    (3, (("variant", 3), ("key12", 1)), "TT", "rs", dict(wave128=True)),
                                                    (4, (("key8", 1),), "TT", "rs_f32", {}), (0, (), "NN", "bias", dict(f32=True))]):
        shape = (304, 264, 3136) if not extra.get("f32") else (70, 136, 1056)
        C.append(_case(f"exactws-f{fam}", fam, shape, lay, epi, kn, i, splitk=True, split=True, exact_ws=True, **extra))
    # ---- family 5: few rows, weights streamed once (per-call policy key 11 = 384; NN only). Every K it covers x every tile the launcher
    # accepts and its own choice; M and N rotate underneath
    Ms, Ns, e5 = [1, 2, 63, 64, 65, 193, 384], [16, 24, 1000], ["plain", "bias", "relu", "half", "f32", "two_bias", "relu_nb"]
    pick = lambda j, N: "relu_nb" if (e5[j % 7] == "relu" and N < 1000) else e5[j % 7]
    i = 0
    for K in (512, 768, 1024, 3072, 4096):
        for tile in ("4,1", "4,2", "4,4", "8,1", "8,2", "auto"):
            for rep in range(2):
                M, N = Ms[(i * 3 + rep) % 7], Ns[(i + rep) % 3]
                C.append(_case(f"f5-tile{tile.replace(',', 'x')}", 5, (M, N, K), "NN", pick(i, N), (("skinny", 384), ("skinny_tile", tile)), i))
                i += 1
    for i, M in enumerate(Ms):         # every M on every N once more under the launcher's own tile choice
        for j, N in enumerate(Ns):
            C.append(_case("f5-tileauto", 5, (M, N, (512, 768, 1024)[(i + j) % 3]), "NN", pick(i + 2 * j, N), (("skinny", 384), ("skinny_tile", "auto")), i + j + 1))
    # what family 5 does not serve goes elsewhere: the other layouts, more rows than the policy's limit, a K it does not cover
    for i, (shape, lay, fam) in enumerate([((64, 24, 768), "NT", 1), ((64, 24, 768), "TN", 1), ((64, 24, 768), "TT", 1), ((385, 24, 768), "NN", 1),
                                           ((64, 24, 1280), "NN", 1), ((64, 8, 768), "NN", 1)]):
        C.append(_case("f5-elsewhere", fam, shape, lay, "bias", (("skinny", 384),), i))
    # ... and an epilogue it does not have (C +=, a second output, an act' operand) runs on family 1 although the policy answers 5
    for i, epi in enumerate(["acc", "relu_pre", "relu_dsave", "dmul", "drelu"]):
        C.append(_case("f5-epilogue-on-f1", 5, (65, 136, 768), "NN", epi, (("skinny", 384),), i))
    out, seen = [], set()
    for c in C:                     # the rotations may meet the same combination twice: keep one
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out


CASES = _build_cases()
# run-to-run: one case each from the split-K, raster and deferred groups (the deferred one is in test_deferred_grouped_reduction)
TWICE = [c for c in CASES if c.name.startswith("split-f3-") and c.rowsum][:1] + \
        [c for c in CASES if c.name.startswith("f3tile") and dict(c.knobs).get("key4") == 2 and c.N > 512][:1]


# ------------------------------------------------------------------------------------------------ the slicing rule, restated
def expected_slices(case, family, ws_bytes):
    """gemm_impl's split-K rule (csrc/gemm.hip) for the workspace offered; family as valor_gemm_kernel_for answers"""
    M, N, K = case.M, case.N, case.K
    if not case.splitk:
        return 1
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if case.f32 or family == 0:
        bk = 32 if case.f32 else 64
        nk = (K + bk - 1) // bk
        s = 1
        if tiles < 512 and nk >= 32:
            s = min((1024 + tiles - 1) // tiles, max(nk // 8, 1), 64)
            while s > 1 and s * M * N * 4 > ws_bytes:
                s -= 1
        steps = (nk + s - 1) // s
        return (nk + steps - 1) // steps if s > 1 else 1
    nk = (K + 63) // 64
    tiles_x = {3: ((M + 255) // 256) * ((N + 255) // 256), 4: ((M + 255) // 256) * ((N + 127) // 128)}.get(family, tiles)
    slots = {3: 256, 4: 512}.get(family, 1024)
    s = 1
    if 2 * tiles_x <= slots and nk >= 24:
        sl = min(slots // tiles_x, nk // 6, 64)
        while sl > 1 and sl * M * N * 4 > ws_bytes:
            sl -= 1
        if sl >= 2:
            s = sl
    if case.rowsum and s > 1:
        while s > 1 and (s * M * N + s * M) * 4 > ws_bytes:
            s -= 1
    return s


def exact_ws_floats(case, family):
    s = expected_slices(case, family, 1 << 40)
    return s, s * case.M * case.N + (s * case.M if case.rowsum else 0)


def runs_on_family(case):
    """family 5 serves plain / bias / activation / alpha / fp32-output epilogues only; gemm_impl runs the rest on the 128x128 kernel"""
    if case.family == 5 and (case.acc or case.preact or case.aux or case.act & ACT_DERIV):
        return 1
    return case.family


# ------------------------------------------------------------------------------------------------ knobs
class Knobs:
    """sets tuning hooks, remembers what they were, puts everything back (teardown of the `knobs` fixture)"""
    SETTERS = {"variant": "valor_gemm_set_variant", "tr_asm": "valor_gemm_set_tr_asm", "fast_epi": "valor_gemm_set_fast_epilogue",
               "sched": "valor_gemm_set_8ph_sched", "nsched": "valor_gemm_set_narrow_sched"}

    def __init__(self, so):
        self.so, self.undo, self.env = so, [], os.environ.get("VALOR_SKINNY_TILE")
        self.policy = None

    def apply(self, knobs):
        for name, value in knobs:
            if name == "skinny":
                from valor_amd import lib
                self.policy = lib.GemmPolicy.make(skinny=value)
            elif name == "skinny_tile":
                if value == "auto":
                    os.environ.pop("VALOR_SKINNY_TILE", None)
                else:
                    os.environ["VALOR_SKINNY_TILE"] = value
            elif name.startswith("key"):
                k = int(name[3:])
                self.undo.append((self.so.valor_gemm_set_policy, (k, self.so.valor_gemm_set_policy(k, value))))
            else:
                fn = getattr(self.so, self.SETTERS[name])
                self.undo.append((fn, (fn(value),)))

    def restore(self):
        for fn, args in reversed(self.undo):
            fn(*args)
        self.undo, self.policy = [], None
        if self.env is None:
            os.environ.pop("VALOR_SKINNY_TILE", None)
        else:
            os.environ["VALOR_SKINNY_TILE"] = self.env


def _snapshot(so):
    return [so.valor_gemm_set_policy(k, -1) for k in range(13)] + [so.valor_gemm_set_variant(-1), so.valor_gemm_set_tr_asm(-1),
            so.valor_gemm_set_fast_epilogue(-1), so.valor_gemm_set_8ph_sched(-1), so.valor_gemm_set_narrow_sched(-1), os.environ.get("VALOR_SKINNY_TILE")]


@pytest.fixture
def knobs(dev):
    from valor_amd import kernels as Kn, lib
    so = lib.load()
    before = _snapshot(so)
    armed = Kn.ReduceQueue._armed
    k = Knobs(so)
    yield k
    k.restore()
    Kn.ReduceQueue._armed = armed
    assert _snapshot(so) == before, "a tuning hook was left changed"


# ------------------------------------------------------------------------------------------------ one call
def _padded(t, dtype, dev):
    """`t` as the leading columns of a wider buffer whose padding holds NaN; the leading dimension stays a multiple of the 16-byte chunk"""
    unit = 8 if dtype == torch.bfloat16 else 4
    rows, cols = t.shape
    ld = (cols + unit - 1) // unit * unit + unit
    buf = torch.full((rows, ld), float("nan"), dtype=dtype, device=dev)
    buf[:, :cols] = t.to(dtype).to(dev)
    return buf[:, :cols]


def family_of(so, case, policy=None):
    dt = 1 if case.f32 else 0
    args = (dt, int(case.ta), int(case.tb), case.M, case.N, case.K, int(case.heavy))
    if policy is not None:
        return so.valor_gemm_kernel_for_tuned(ctypes.addressof(policy), *args)
    return so.valor_gemm_kernel_for(*args)


def run_case(case, dev, knobs):
    """builds the operands, checks the conditions, pins and asserts the kernel, runs valor_gemm into guarded buffers; returns what `check`
    compares"""
    from valor_amd import kernels as Kn, lib
    so = knobs.so
    ref = GE.case_reference(case)
    GE.check_exactness_conditions(case, ref)
    knobs.apply(case.knobs)
    fam = family_of(so, case, knobs.policy)
    assert fam == case.family, f"{case.name}: valor_gemm_kernel_for answers {fam}, the case means family {case.family}"
    w128 = so.valor_gemm_wave128_for(0, int(case.ta), int(case.tb), case.M, case.N, case.K, int(case.heavy)) if not case.f32 else 0
    assert bool(w128) == case.wave128, f"{case.name}: valor_gemm_wave128_for answers {w128}"
    fam_run = runs_on_family(case)
    dt = torch.float32 if case.f32 else torch.bfloat16
    odt = torch.float32 if (case.f32 or case.out_f32) else torch.bfloat16
    M, N, K = case.M, case.N, case.K
    A, B = _padded(ref["A"], dt, dev), _padded(ref["B"], dt, dev)
    bias = ref["bias"].to(dt).to(dev) if ref["bias"] is not None else None
    aux = None
    if ref["aux"] is not None:                      # its own leading dimension (the same residue mod 8 as ldc, so the wide paths stay reachable)
        abuf = torch.full((M, N + case.ld_extra + 8), float("nan"), dtype=dt, device=dev)
        aux = abuf[:, :N]
        aux.copy_(ref["aux"].to(dt))
    cbuf, c = GE.guarded(M, N, odt, dev, case.ld_extra, prefill=not case.acc)
    if case.acc:
        c.copy_(ref["C0"].to(odt))
    pbuf = p = None
    if case.preact:
        pbuf, p = GE.guarded(M, N, odt, dev, case.ld_extra)
    rbuf = r = None
    if case.rowsum:
        rbuf, r = GE.guarded(M, None, odt, dev, 0, prefill=case.rowsum != "acc")
        if case.rowsum == "acc":
            r.copy_(ref["r0"].to(odt))
    wsbuf = ws = None
    ws_bytes = 0
    if case.splitk:
        if case.exact_ws:
            _, n = exact_ws_floats(case, fam_run)
            wsbuf = torch.full((n + 128,), 7.25, dtype=torch.float32, device=dev)
            ws, ws_bytes = wsbuf[64:64 + n], n * 4
        else:
            ws = Kn.workspace(dev)
            ws_bytes = ws.numel() * 4
        slices = expected_slices(case, fam_run, ws_bytes)
        assert (slices > 1) == case.split, f"{case.name}: the slicing rule gives {slices} slices"
    direct = case.preact or case.exact_ws
    if not direct:
        got = Kn.gemm(A, B, trans_a=case.ta, trans_b=case.tb, bias=bias, act=case.act, dact_aux=aux, alpha=case.alpha, out=c,
                      accumulate=case.acc, out_dtype=odt, splitk=case.splitk, rowsum_out=r, rowsum_accumulate=case.rowsum == "acc",
                      policy=knobs.policy)
        assert got.data_ptr() == c.data_ptr()
    else:
        args = (torch.cuda.current_stream().cuda_stream, 1 if case.f32 else 0, int(case.ta), int(case.tb), M, N, K, A.data_ptr(), A.stride(0),
                B.data_ptr(), B.stride(0), c.data_ptr(), c.stride(0), bias.data_ptr() if bias is not None else 0, case.act,
                p.data_ptr() if p is not None else 0, aux.data_ptr() if aux is not None else 0, aux.stride(0) if aux is not None else 0,
                float(case.alpha), int(case.acc), int(case.out_f32), ws.data_ptr() if ws is not None else 0, ws_bytes,
                r.data_ptr() if r is not None else 0, int(case.rowsum == "acc"))
        if knobs.policy is not None:
            lib.call("valor_gemm_tuned", ctypes.addressof(knobs.policy), *args)
        else:
            lib.call("valor_gemm", *args)
    torch.cuda.synchronize()
    return dict(ref=ref, C=(cbuf, c), preact=(pbuf, p), rowsum=(rbuf, r), ws=(wsbuf, ws))


def check(case, res):
    ref = res["ref"]
    for key in ("C", "preact", "rowsum"):
        buf, view = res[key]
        if view is None:
            continue
        try:
            GE.compare(view, ref[key], buf, view)
        except GE.Mismatch as e:
            raise AssertionError(f"{case.name}: {key}\n{e}") from None
    wsbuf, ws = res["ws"]
    if wsbuf is not None:           # the floats on either side of the exact piece keep their pattern
        n = ws.numel()
        assert bool((wsbuf[:64] == 7.25).all()) and bool((wsbuf[64 + n:] == 7.25).all()), f"{case.name}: the workspace piece was overrun"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_exact(case, dev, knobs):
    check(case, run_case(case, dev, knobs))


@pytest.mark.parametrize("case", TWICE, ids=[c.name for c in TWICE])
def test_run_to_run(case, dev, knobs):
    """the same call twice in one process: the same bits, guards included"""
    first = run_case(case, dev, knobs)
    knobs.restore()
    second = run_case(case, dev, knobs)
    check(case, first)
    check(case, second)
    for key in ("C", "preact", "rowsum"):
        if first[key][0] is not None:
            a, b = first[key][0], second[key][0]
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                               b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), (case.name, key)


# ------------------------------------------------------------------------------------------------ deferred, grouped reductions
# (Mo, No, Kt, accumulate, row sums, fp32 out): wgrads dY^T.X under the default policy -- family 3 from K = 4096 (four-wave kernel above 48
# K-tiles per workgroup), family 1 below; the sixth is too short to be split and completes at once
DEFERRED = [(304, 520, 4160, True, "acc", False), (257, 264, 4096, False, "plain", False), (520, 264, 3136, True, "", False),
            (264, 300, 4160, False, "", True), (128, 136, 3200, True, "", False), (304, 264, 448, False, "", False),
            (1000, 328, 4096, True, "acc", True), (70, 136, 1600, False, "", False)]
NINTH = [(256, 256, 4096, True, "plain", False), (129, 260, 1664, True, "", False)]


def _deferred_cases(specs):
    out = []
    for i, (M, N, K, acc, rs, f32o) in enumerate(specs):
        fam = 3 if (K >= 4096 and M >= 256 and N >= 256) else 1
        out.append(Case(name=f"deferred-{M}x{N}x{K}", family=fam, M=M, N=N, K=K, ta=True, tb=True, acc=acc, rowsum=rs, out_f32=f32o,
                        splitk=True, split=K >= 1536, ld_extra=LD_EXTRA[i % 3], seed=1 + i % 2))
    return out


DEFERRED_CASES = _deferred_cases(DEFERRED) + _deferred_cases(NINTH)


def _queue_deferred(case, dev, so, order):
    from valor_amd import kernels as Kn
    ref = GE.case_reference(case)
    GE.check_exactness_conditions(case, ref)
    assert family_of(so, case) == case.family
    odt = torch.float32 if case.out_f32 else torch.bfloat16
    A, B = _padded(ref["A"], torch.bfloat16, dev), _padded(ref["B"], torch.bfloat16, dev)
    cbuf, c = GE.guarded(case.M, case.N, odt, dev, case.ld_extra, prefill=not case.acc)
    if case.acc:
        c.copy_(ref["C0"].to(odt))
    rbuf = r = None
    if case.rowsum:
        rbuf, r = GE.guarded(case.M, None, odt, dev, 0, prefill=case.rowsum != "acc")
        if case.rowsum == "acc":
            r.copy_(ref["r0"].to(odt))
    Kn.gemm(A, B, trans_a=True, trans_b=True, out=c, accumulate=case.acc, out_dtype=odt, rowsum_out=r, rowsum_accumulate=case.rowsum == "acc",
            defer_done=lambda: order.append(case.name))
    return dict(ref=ref, C=(cbuf, c), preact=(None, None), rowsum=(rbuf, r), ws=(None, None), keep=(A, B))


def _deferred_round(dev, knobs, cases):
    from valor_amd import kernels as Kn
    order, res = [], []
    Kn.ReduceQueue._armed = True                 # as inside a backward pass: nothing flushes until the end-of-backward callback
    try:
        q = Kn.ReduceQueue.current(dev)
        assert q.n == 0 and q.GROUP == 8
        pending = 0
        for case in cases:
            res.append(_queue_deferred(case, dev, knobs.so, order))
            if case.split:
                pending += 1
                if pending > q.GROUP:            # the ninth split product: the queue closed its first group by itself
                    assert q.n == pending - q.GROUP and len(order) == len(cases[:len(res)]) - q.n
                else:
                    assert q.n == pending
            else:
                assert order[-1] == case.name    # not split: complete at once
    finally:
        Kn.ReduceQueue.flush_all()
    torch.cuda.synchronize()
    assert q.n == 0 and sorted(order) == sorted(c.name for c in cases)
    for case, r in zip(cases, res):
        check(case, r)
    return res


def test_deferred_grouped_reduction(dev, knobs):
    """eight wgrads of different shapes through kernels.ReduceQueue (valor_gemm_deferred + ONE valor_gemm_reduce_group): some with fused row
    sums, some accumulating, fp32 and bf16 outputs, one not split; every output equals the integer reference, every guard is intact. Then the
    same with two more split products, so that the ninth closes the first group by itself. The first round runs twice: the same bits."""
    eight = DEFERRED_CASES[:8]
    assert sum(c.split for c in eight) == 7
    first = _deferred_round(dev, knobs, eight)
    second = _deferred_round(dev, knobs, eight)
    for a, b in zip(first, second):
        for key in ("C", "rowsum"):
            if a[key][0] is not None:
                assert torch.equal(a[key][0].float(), b[key][0].float())
    _deferred_round(dev, knobs, DEFERRED_CASES)


def coverage(so=None):
    """what the table reaches, from the switches each case sets (and, with the library, from what valor_gemm_kernel_for answers):
    {(family, kernel, layout, schedule, epilogue path, split): number of cases}"""
    from collections import Counter
    out = Counter()
    for c in CASES + DEFERRED_CASES:
        kn = dict(c.knobs)
        fam = runs_on_family(c)
        lay = ("T" if c.ta else "N") + ("T" if c.tb else "N")
        split = c.split
        tile_ok = (not c.out_f32 and not split and c.N % 8 == 0 and (c.N + c.ld_extra) % 8 == 0 and not c.rowsum and not c.ta
                   and not (c.aux and c.preact) and not (c.preact and c.act & ACT_DERIV))
        fe = kn.get("fast_epi", 1)
        plainish = fe >= 2 or (not c.preact and (not c.aux or c.aux == "deriv"))
        kernel, sched, epi = f"f{fam}", "-", "general"
        fused = bool(c.act & 15 or c.preact or c.aux)
        if fam in (1, 2):
            epi = "reduce" if split else ("fused" if fused else "lean")
        elif fam == 0:
            kernel, epi = ("f0-fp32" if c.f32 else "f0-bf16"), ("reduce" if split else "general")
        elif fam == 3:
            if c.wave128:
                kernel, sched = "f3-four-wave", f"sched{kn.get('sched', 1000)}"
            else:
                kernel = "f3-eight-wave"
                sched = f"sched{kn.get('sched', 1000)}" + (f"-asm{kn.get('tr_asm', 1)}" if (c.ta or c.tb) else "")
                epi = "tile" if (fe and plainish and tile_ok) else "general"
            epi = "reduce" if split else epi
        elif fam == 4:
            wide = lay == "NN" and not split and not c.rowsum and kn.get("key10", 0)
            kernel = "f4-wide" if wide else ("f4-mfma32" if (lay == "NN" and kn.get("key9", 0)) else "f4")
            sched = "-" if wide else f"sched{kn.get('nsched', 1)}" + (f"-asm{kn.get('tr_asm', 1)}" if (c.ta or c.tb) else "")
            epi = "reduce" if split else ("tile" if (fe and plainish and tile_ok) else "general")
        elif fam == 5:
            kernel = "f5-tile" + kn.get("skinny_tile", "auto")
        out[(fam, kernel, lay, sched, epi, "split" if split else "whole")] += 1
    return out
