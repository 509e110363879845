"""The grouped weight-gradient launch (valor_gemm_group, kernels.ReduceQueue under VALOR_GROUP_WGRAD): several  C += A^T . B  products of
one layer as ONE split-K launch with a common slice plan, then one grouped reduction.

Checked:
  1. exact inputs at tolerance zero (tests/gemm_exact.py: operands in {-1, 0, 1} whose partial sums over ANY K range are bf16 integers, so
     every slicing has the same answer): groups of 1, 2, 3 (1 + 3 + 9 tiles), 8 and 9 products (9 = two flushes), with an edge tile, a
     65-K-tile contraction (uneven slices), two contraction lengths in one group, fused row sums fresh and accumulating, C += onto a
     prefilled C; against the fp64 reference AND against the ungrouped K.gemm, on both kernels (policy key 12 = 0 / 1);
  2. random bf16 inputs: the error against fp64 of the grouped and of the ungrouped path, both within an a-priori bound;
  3. the same C twice in a row closes the group: two sequential accumulations;
  4. a write into a queued product's operand flushes the queue first: the product used the operand's old value;
  5. ReduceQueue.discard_stale drops queued products: the target stays untouched;
  6. two decoder layers (hidden 256, 4096 rows) with the switch on and off: parameter gradients against fp64 autograd within the tolerance
     of tests/test_param_grad_paths_gpu.py, the switch-on run byte-identical twice.
The operands' exactness conditions are checked on the CPU in the fixture (and in tests/test_gemm_group_plan_cpu.py without a GPU).
"""
import contextlib
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_exact as GE  # noqa: E402

pytestmark = pytest.mark.gpu

BUDGET = 32
# (M, N, K, rowsum): 1 / 3 / 9 / 2 / 2 / 1 / 4 / 3 / 1 tiles of 256 x 256; 320 = an edge tile; 4160 = 65 K-tiles; 8832 = the decoder's contraction
PROBLEMS = [(256, 256, 4096, ""), (768, 256, 4096, "plain"), (768, 768, 4160, ""), (320, 256, 4096, "acc"), (256, 320, 8832, ""),
            (256, 256, 4160, ""), (320, 320, 4096, ""), (256, 768, 4096, ""), (256, 256, 4096, "")]
GROUPS = {"1": [0], "2": [0, 1], "3": [0, 1, 2], "8": list(range(8)), "9": list(range(9)), "mixedK": [3, 4, 2]}
GRAD_TOL = 1.2e-2            # tests/test_param_grad_paths_gpu.py, bf16


def case_of(i):
    M, N, K, rs = PROBLEMS[i]
    return GE.Case(f"group_p{i}", 3, M, N, K, ta=True, tb=True, acc=True, rowsum=rs, splitk=True, seed=11 + i, budget=BUDGET)


def exact_problem(i):
    """the CPU side of problem i: operands, C0, r0, the reference outputs; the exactness conditions hold for every contiguous K range"""
    case = case_of(i)
    ref = GE.case_reference(case)
    GE.check_exactness_conditions(case, ref)
    return case, ref


@pytest.fixture(scope="module")
def problems(dev):
    """every problem once: reference on the CPU, operands on the device, and the ungrouped K.gemm result"""
    from valor_amd import kernels as K, lib
    so = lib.load()
    out = []
    for i in range(len(PROBLEMS)):
        case, ref = exact_problem(i)
        assert so.valor_gemm_kernel_for(lib.DT_BF16, 1, 1, case.M, case.N, case.K, 0) == 3, case
        a, b = ref["A"].to(torch.bfloat16).to(dev), ref["B"].to(torch.bfloat16).to(dev)
        p = dict(case=case, ref=ref, a=a, b=b)
        c, r = fresh_outputs(p, dev)
        K.gemm(a, b, trans_a=True, trans_b=True, out=c["view"], accumulate=True, rowsum_out=r and r["view"], rowsum_accumulate=case.rowsum == "acc")
        torch.cuda.synchronize()
        GE.compare(c["view"], ref["C"], c["buf"], c["view"])
        p["alone"] = (c["view"].clone(), r["view"].clone() if r else None)
        out.append(p)
    return out


def fresh_outputs(p, dev):
    """guarded C (prefilled with C0) and row-sum vector (prefilled with r0, or the `unwritten` canary when the sums are fresh)"""
    case, ref = p["case"], p["ref"]
    buf, view = GE.guarded(case.M, case.N, torch.bfloat16, dev, case.ld_extra, prefill=False)
    view.copy_(ref["C0"].to(torch.bfloat16))
    r = None
    if case.rowsum:
        rbuf, rview = GE.guarded(case.M, None, torch.bfloat16, dev, 0, prefill=True)
        if case.rowsum == "acc":
            rview.copy_(ref["r0"].to(torch.bfloat16))
        r = dict(buf=rbuf, view=rview)
    return dict(buf=buf, view=view), r


@contextlib.contextmanager
def switch(on, key12=None):
    """VALOR_GROUP_WGRAD for the duration (the class attribute the env variable presets), optionally policy key 12 (0: eight-wave loop, 1:
    four-wave loop for every family-3 wgrad and every group)"""
    from valor_amd import kernels as K, lib
    so = lib.load()
    old, K.ReduceQueue.group_wgrad = K.ReduceQueue.group_wgrad, on
    old12 = so.valor_gemm_set_policy(12, key12) if key12 is not None else None
    try:
        yield
    finally:
        K.ReduceQueue.flush_all()
        K.ReduceQueue.group_wgrad = old
        if old12 is not None:
            so.valor_gemm_set_policy(12, old12)


@contextlib.contextmanager
def launches():
    """names of the lib.call entries made inside"""
    from valor_amd import lib
    names, real = [], lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    lib.call = call
    try:
        yield names
    finally:
        lib.call = real


def issue(K, p, c, r, done):
    case = p["case"]
    K.gemm(p["a"], p["b"], trans_a=True, trans_b=True, out=c["view"], accumulate=True, rowsum_out=r and r["view"],
           rowsum_accumulate=case.rowsum == "acc", defer_done=lambda: done.append(case.name))


def plan_of(idx):
    from valor_amd import lib
    n = len(idx)
    shapes = (ctypes.c_int * (4 * n))(*[v for i in idx for v in (PROBLEMS[i][0], PROBLEMS[i][1], PROBLEMS[i][2], int(bool(PROBLEMS[i][3])))])
    slices, info = (ctypes.c_int * n)(), (ctypes.c_int * 4)()
    lib.call("valor_gemm_group_plan", ctypes.cast(shapes, ctypes.c_void_p), n, ctypes.cast(slices, ctypes.c_void_p), None, ctypes.cast(info, ctypes.c_void_p))
    return list(slices), list(info)


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("key12", [0, 1], ids=["eight_wave", "four_wave"])
@pytest.mark.parametrize("group", list(GROUPS), ids=list(GROUPS))
def test_exact_groups(dev, problems, group, key12):
    from valor_amd import kernels as K
    idx = GROUPS[group]
    outs, done = [], []
    with switch(True, key12), launches() as names:
        slices, info = plan_of(idx[:8])
        names.clear()
        with K.ReduceQueue.batch():
            for i in idx:
                c, r = fresh_outputs(problems[i], dev)
                outs.append((c, r))
                issue(K, problems[i], c, r, done)
            # nothing is reported before its flush; the ninth product closed the group of the first eight
            assert done == ([problems[i]["case"].name for i in idx[:8]] if len(idx) > 8 else [])
        torch.cuda.synchronize()
    nflush = (len(idx) + 7) // 8
    assert names.count("valor_gemm_group") == nflush and names.count("valor_gemm_reduce_group") <= nflush, names
    assert not any(n in ("valor_gemm", "valor_gemm_deferred") for n in names), names          # every product went through the group
    assert done == [problems[i]["case"].name for i in idx]
    print(f"group {group}: slices {slices}, {info[0]} work items, shortest K loop {info[1]} K-tiles, four-wave kernel {info[2]}")
    assert info[2] == key12 and info[0] <= 256 and max(slices) > 1
    for i, (c, r) in zip(idx, outs):
        p = problems[i]
        GE.compare(c["view"], p["ref"]["C"], c["buf"], c["view"])                      # the integer reference, guards untouched
        assert torch.equal(c["view"], p["alone"][0]), p["case"].name                    # the ungrouped K.gemm, element for element
        if r is not None:
            GE.compare(r["view"], p["ref"]["rowsum"], r["buf"], r["view"])
            assert torch.equal(r["view"], p["alone"][1]), p["case"].name


# ------------------------------------------------------------------------------------------------ 2. random inputs
def test_random_inputs_error_bound(dev):
    """A-priori bound per element, for ANY slice count S: every partial is rounded to bf16 once (relative 2^-9 of |partial_s|, and
    sum_s |partial_s| <= (|A|^T |B|)[m, n] =: P), the sum + C0 is rounded to bf16 once (2^-9 of |result| <= P + |C0|), and the fp32
    accumulations add at most (K + S) 2^-24 P (S <= 64):  |err| <= (2 * 2^-9 + (K + 64) * 2^-24) * P + 2^-9 * |C0|."""
    from valor_amd import kernels as K
    shapes = [(768, 768, 4160), (256, 320, 4096), (320, 256, 8832)]
    g = torch.Generator().manual_seed(5)
    ops_, c0s = [], []
    for M, N, Kd in shapes:
        ops_.append((torch.randn((Kd, M), generator=g).to(torch.bfloat16).to(dev), torch.randn((Kd, N), generator=g).to(torch.bfloat16).to(dev)))
        c0s.append(torch.randn((M, N), generator=g).to(torch.bfloat16).to(dev))
    alone = [c.clone() for c in c0s]
    for (a, b), c in zip(ops_, alone):
        K.gemm(a, b, trans_a=True, trans_b=True, out=c, accumulate=True)
    grouped = [c.clone() for c in c0s]
    with switch(True), launches() as names:
        with K.ReduceQueue.batch():
            for (a, b), c in zip(ops_, grouped):
                K.gemm(a, b, trans_a=True, trans_b=True, out=c, accumulate=True, defer_done=lambda: None)
        torch.cuda.synchronize()
    assert names.count("valor_gemm_group") == 1 and "valor_gemm_deferred" not in names, names
    for (M, N, Kd), (a, b), c0, ca, cg in zip(shapes, ops_, c0s, alone, grouped):
        a64, b64 = a.double(), b.double()
        exact = a64.t() @ b64 + c0.double()
        bound = (2 * 2.0 ** -9 + (Kd + 64) * 2.0 ** -24) * (a64.abs().t() @ b64.abs()) + 2.0 ** -9 * c0.double().abs()
        ea, eg = (ca.double() - exact).abs(), (cg.double() - exact).abs()
        print(f"{M}x{N}x{Kd}: max err ungrouped {float(ea.max()):.4f} ({float((ea / bound).max()):.3f} of the bound), "
              f"grouped {float(eg.max()):.4f} ({float((eg / bound).max()):.3f} of the bound)")
        assert bool((ea <= bound).all()) and bool((eg <= bound).all())


# ------------------------------------------------------------------------------------------------ 3. repeated target
def test_repeated_target_closes_the_group(dev, problems):
    from valor_amd import kernels as K
    p, q = problems[0], problems[8]                     # the same shape, different operands
    c, _ = fresh_outputs(p, dev)
    done = []
    with switch(True), launches() as names:
        with K.ReduceQueue.batch():
            issue(K, p, c, None, done)
            issue(K, q, c, None, done)
            assert done == [p["case"].name]                     # the second product closed the first one's group
        torch.cuda.synchronize()
    assert names.count("valor_gemm_group") == 2, names
    want = p["ref"]["C"] + (q["ref"]["C"] - q["ref"]["C0"])
    assert float(want.abs().max()) <= 256.0                     # still exact in bf16
    GE.compare(c["view"], want, c["buf"], c["view"])


# ------------------------------------------------------------------------------------------------ 4. overwrite guard
def test_write_into_a_queued_operand_flushes_first(dev, problems):
    from valor_amd import kernels as K
    p = problems[0]
    a = p["a"].clone()                                   # [K, M]: the operand a later GEMM accumulates into
    c, _ = fresh_outputs(p, dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-1, 2, (a.shape[0], 64), generator=g).to(torch.bfloat16).to(dev)
    y = torch.randint(-1, 2, (a.shape[1], 64), generator=g).to(torch.bfloat16).to(dev)
    done = []
    with switch(True), launches() as names:
        with K.ReduceQueue.batch():
            K.gemm(a, p["b"], trans_a=True, trans_b=True, out=c["view"], accumulate=True, defer_done=lambda: done.append(1))
            assert done == [] and "valor_gemm_group" not in names
            K.gemm(x, y, out=a, accumulate=True)         # a += x y^T
            assert done == [1] and names.index("valor_gemm_group") < names.index("valor_gemm")
        torch.cuda.synchronize()
    assert not torch.equal(a, p["a"])                            # the operand did change ...
    GE.compare(c["view"], p["ref"]["C"], c["buf"], c["view"])    # ... and the queued product read its old value


# ------------------------------------------------------------------------------------------------ 5. stale queue
def test_discard_stale_drops_queued_products(dev, problems):
    from valor_amd import kernels as K
    p = problems[0]
    c, _ = fresh_outputs(p, dev)
    before = c["buf"].clone()
    done = []
    with switch(True), launches() as names:
        with K.ReduceQueue.batch():
            issue(K, p, c, None, done)
            assert K.ReduceQueue._nqueued == 1
            assert K.ReduceQueue.discard_stale()
            assert K.ReduceQueue._nqueued == 0
        torch.cuda.synchronize()
    assert "valor_gemm_group" not in names and "valor_gemm_reduce_group" not in names, names
    assert done == [] and torch.equal(c["buf"], before)


# ------------------------------------------------------------------------------------------------ 6. two decoder layers
HID, HEADS, ROWS_B, ROWS_S, SKV, INTER = 256, 4, 32, 128, 64, 1024
LAYER_PARAMS = [("qkv.w", (3 * HID, HID)), ("qkv.b", (3 * HID,)), ("o.w", (HID, HID)), ("o.b", (HID,)), ("ln1.w", (HID,)), ("ln1.b", (HID,)),
                ("cq.w", (HID, HID)), ("cq.b", (HID,)), ("co.w", (HID, HID)), ("co.b", (HID,)), ("ln2.w", (HID,)), ("ln2.b", (HID,)),
                ("fc1.w", (INTER, HID)), ("fc1.b", (INTER,)), ("fc2.w", (HID, INTER)), ("fc2.b", (HID,)), ("ln3.w", (HID,)), ("ln3.b", (HID,))]


def _stack_inputs(dev):
    g = torch.Generator().manual_seed(77)
    P = {}
    for layer in range(2):
        for name, shape in LAYER_PARAMS:
            if name.startswith("ln") and name.endswith(".w"):
                t = 1.0 + 0.1 * torch.randn(shape, generator=g)
            elif len(shape) == 2:
                t = torch.randn(shape, generator=g) * shape[1] ** -0.5
            else:
                t = 0.1 * torch.randn(shape, generator=g)
            P[f"{layer}.{name}"] = t.to(torch.bfloat16).to(dev)
    x = torch.randn((ROWS_B, ROWS_S, HID), generator=g).to(torch.bfloat16).to(dev)
    kv = torch.randn((ROWS_B, SKV, 2 * HID), generator=g).to(torch.bfloat16).to(dev)
    dy = torch.randn((ROWS_B, ROWS_S, HID), generator=g).to(torch.bfloat16).to(dev)
    return P, x, kv, dy


def _stack_valor(P, x, kv, dy):
    """the decoder's post-LN layer (model/valor.py bert_encoder) twice; parameter gradients accumulate into arena-like slots"""
    from valor_amd import lib, ops
    leaves = {}
    for k, t in P.items():
        p = t.clone().requires_grad_(True)
        p._arena_name = k
        p.grad = torch.zeros_like(t)
        leaves[k] = p
    seen = []
    old, ops.GradSink.listener = ops.GradSink.listener, seen.append
    try:
        h = x.clone().requires_grad_(True)
        y = h
        for i in range(2):
            L = lambda n: leaves[f"{i}.{n}"]          # noqa: E731
            qkv = ops.linear(y, L("qkv.w"), L("qkv.b"))
            a = ops.self_attention(qkv, HEADS, None, 0.0)
            o = ops.linear(a, L("o.w"), None)
            y = ops.bias_dropout_residual_ln(o, L("o.b"), y, L("ln1.w"), L("ln1.b"), 1e-12, 0.0, False)
            cq = ops.linear(y, L("cq.w"), L("cq.b"))
            c = ops.cross_attention(cq, kv, HEADS, None, 0, 0.0)
            o = ops.linear(c, L("co.w"), None)
            y = ops.bias_dropout_residual_ln(o, L("co.b"), y, L("ln2.w"), L("ln2.b"), 1e-12, 0.0, False)
            m = ops.mlp(y, L("fc1.w"), L("fc1.b"), L("fc2.w"), None, lib.ACT_GELU_ERF)
            y = ops.bias_dropout_residual_ln(m, L("fc2.b"), y, L("ln3.w"), L("ln3.b"), 1e-12, 0.0, False)
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        ops.GradSink.listener = old
    return {k: p.grad.clone() for k, p in leaves.items()}, h.grad.clone(), seen


def _attn64(q, k, v):
    B, S, E = q.shape
    sp = lambda t: t.view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)         # noqa: E731
    w = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / 8.0, dim=-1)
    return (w @ sp(v)).transpose(1, 2).reshape(B, S, E)


def _stack_ref(P, x, kv, dy):
    L64 = {k: t.double().requires_grad_(True) for k, t in P.items()}
    y, kv64 = x.double(), kv.double()
    for i in range(2):
        W = lambda n: L64[f"{i}.{n}"]          # noqa: E731
        qkv = y @ W("qkv.w").t() + W("qkv.b")
        a = _attn64(qkv[..., :HID], qkv[..., HID:2 * HID], qkv[..., 2 * HID:])
        y = F.layer_norm(a @ W("o.w").t() + W("o.b") + y, (HID,), W("ln1.w"), W("ln1.b"), 1e-12)
        cq = y @ W("cq.w").t() + W("cq.b")
        c = _attn64(cq, kv64[..., :HID], kv64[..., HID:])
        y = F.layer_norm(c @ W("co.w").t() + W("co.b") + y, (HID,), W("ln2.w"), W("ln2.b"), 1e-12)
        m = F.gelu(y @ W("fc1.w").t() + W("fc1.b")) @ W("fc2.w").t() + W("fc2.b")
        y = F.layer_norm(m + y, (HID,), W("ln3.w"), W("ln3.b"), 1e-12)
    y.backward(dy.double())
    return {k: t.grad for k, t in L64.items()}


def test_two_decoder_layers_switch_on_and_off(dev):
    P, x, kv, dy = _stack_inputs(dev)
    ref = _stack_ref(P, x, kv, dy)
    runs = {}
    for name, on in (("off", False), ("on", True), ("on_again", True)):
        with switch(on), launches() as names:
            runs[name] = _stack_valor(P, x, kv, dy) + (list(names),)
    assert "valor_gemm_group" not in runs["off"][3]
    # the twelve weight gradients (14 tiles per layer) in two launches, 8 + 4: none of them goes through valor_gemm_deferred any more
    assert runs["on"][3].count("valor_gemm_group") == 2 and "valor_gemm_deferred" not in runs["on"][3], runs["on"][3]
    errs = {}
    for name in ("off", "on"):
        grads, dx, seen, _ = runs[name]
        assert sorted(seen) == sorted(P), name                         # every parameter reported once
        for k in P:
            errs[name, k] = float((grads[k].double() - ref[k]).norm() / ref[k].norm().clamp_min(1e-30))
            print(f"{name} d{k} rel {errs[name, k]:.3e} (tol {GRAD_TOL:.1e})")
    for key, e in errs.items():
        assert e < GRAD_TOL, (key, e)
    for k in P:
        assert torch.equal(runs["on"][0][k], runs["on_again"][0][k]), k
    assert torch.equal(runs["on"][1], runs["on_again"][1])
    assert torch.equal(runs["on"][1], runs["off"][1])                  # the activation gradients do not depend on the switch
