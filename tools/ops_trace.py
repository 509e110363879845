#!/usr/bin/env python
"""What the parameter-gradient paths of valor_amd/ops.py launch, report and compute, as one JSON file -- to be run on two commits and
compared (a refactor of ops.py must leave the file unchanged):

    python tools/ops_trace.py OUT.json [--package-root DIR]        # DIR: a checkout whose valor_amd is traced (default: this one)
    python tools/ops_trace.py --compare A.json B.json SUMMARY.json --commits ID_A ID_B

For every case and route of tests/test_param_grad_paths_gpu.py (linear, mlp, the three tied-decoder loss entry points, two nodes on one
GradSlot), for ops.embed / assemble_tokens / bias_dropout_residual on both routes, and for one forward + backward of the pretraining
task on the smallest model tests/test_model_gpu.py builds (fp32 and bf16, dropout on, sinks on), it records
  * the ordered lib.call stream: entry point and every argument whose declared type in lib.SIGNATURES is not a pointer,
  * the ordered names GradSink.listener was told,
  * the SHA-256 of every output and every gradient, returned or arena-resident, after ReduceQueue.flush_all() and a synchronize.
Only names both commits have are used."""
import argparse
import ctypes
import hashlib
import importlib.util
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(t):
    import torch
    if t is None:
        return None
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def _values(lib, calls):
    scalar = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double)
    out = []
    for name, args in calls:
        types = lib.SIGNATURES[name]
        out.append([name] + [a for a, t in zip(args, types) if t in scalar])
    return out


def _entry(lib, r, tensors):
    return {"calls": _values(lib, r["calls"]), "reported": list(r["seen"]), "recorded": list(r.get("recorded", [])),
            "sha256": {k: _sha(v) for k, v in tensors.items()}}


def _op_cases(T, lib, dev):
    out = {}
    for kind, run, cases in (("linear", T.run_linear, T.LINEAR_CASES), ("mlp", T.run_mlp, T.MLP_CASES), ("loss", T.run_loss, T.LOSS_CASES)):
        for case in cases:
            for route in T.ROUTES:
                r = run(dev, case, route)
                outs = r["out"] if isinstance(r["out"], tuple) else (r["out"],)
                tensors = {f"out{i}": o for i, o in enumerate(outs)}
                tensors["dx"] = r["x"][0].grad
                tensors.update({"d" + leaf.name: leaf.p.grad for leaf, _ in r["leaves"]})
                tensors.update({k: r[k] for k in ("rows",) if k in r})
                out[f"{kind}/{T._id(case)}/{route}"] = _entry(lib, r, tensors)
    for op, cases in (("linear", T.LINEAR_CASES), ("mlp", T.MLP_CASES)):
        for case in cases:
            r = T.run_slot(dev, op, case)
            tensors = {"dx": r["x"][0].grad}
            tensors.update({f"out{i}": y for i, y in enumerate(r["outs"])})
            tensors.update({f"d{i}.{j}": p.grad for i, ps in enumerate(r["leaves"]) for j, p in enumerate(ps)})
            out[f"slot/{op}/{T._id(case)}"] = _entry(lib, r, tensors)
    return out


def _glue_cases(T, lib, dev):
    """embed, assemble_tokens and bias_dropout_residual, gradients returned and sunk"""
    import torch
    from valor_amd import ops
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        for route in ("ret", "sink"):
            g = torch.Generator().manual_seed(5)
            B, L, V, E, N, Pn = 3, 7, 50, 64, 5, 3
            ids = torch.randint(0, V, (B, L), generator=g).to(dev)
            mk = lambda shape, name: T.Leaf(T._randn(shape, g, dtype, dev), route, name, g)
            word, pos, typ = mk((V, E), "word"), mk((L + 2, E), "pos"), mk((E,), "type")
            cls, apos, abias = mk((E,), "cls"), mk((Pn + 1, E), "apos"), mk((E,), "abias")
            rbias = mk((E,), "rbias")
            patches = T._randn((N * Pn, E), g, dtype, dev).requires_grad_(True)
            xr, res = (T._randn((B * L, E), g, dtype, dev).requires_grad_(True) for _ in range(2))
            d1, d2, d3 = T._randn((B, L, E), g, dtype, dev), T._randn((N, Pn + 1, E), g, dtype, dev), T._randn((B * L, E), g, dtype, dev)
            ops.DropoutState.reset(77)
            with T.recording(route) as (calls, seen, recorded):
                o1 = ops.embed(ids, word.p, pos.p, typ.p, L)
                o2 = ops.assemble_tokens(patches, cls.p, apos.p, abias.p, N, Pn)
                o3 = ops.bias_dropout_residual(xr, rbias.p, res, 0.1)
                torch.autograd.backward([o1, o2, o3], [d1, d2, d3])
                T._finish()
            tensors = {"o1": o1, "o2": o2, "o3": o3, "dpatches": patches.grad, "dxr": xr.grad, "dres": res.grad}
            tensors.update({"d" + l.name: l.p.grad for l in (word, pos, typ, cls, apos, abias, rbias)})
            out[f"glue/{T._id(dtype)}/{route}"] = _entry(lib, dict(calls=calls, seen=seen, recorded=recorded), tensors)
    return out


def _model_step(T, lib, dev):
    import torch
    from valor_amd import ops, synth
    from valor_amd.model.valor import VALOR
    task = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        spec = synth.tiny_spec()
        sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
        batch = synth.make_batch(spec, batch=2, frames=2, audio_slices=1, txt_len=32, seed=4)
        model = VALOR({"dropout": 0.1, "drop_path_rate": 0.0}, spec=spec, dtype=dtype, device=dev)
        model.load_state_dict(sd, strict=True)
        model.train()
        assert ops.GradSink.enabled
        ops.DropoutState.reset(99)
        random.seed(11)
        with T.recording() as (calls, seen, recorded):
            losses = model(batch, task=task, compute_loss=True)
            sum(losses.values()).backward()
            T._finish()
        tensors = {k: v for k, v in losses.items()}
        tensors.update({"d:" + name: model.P[name].grad for name, _shape, _refs in model.table})
        out[f"model/{T._id(dtype)}"] = _entry(lib, dict(calls=calls, seen=seen, recorded=recorded), tensors)
    return out


def trace(path, package_root):
    sys.path.insert(0, package_root)
    import torch
    from valor_amd import lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(lib.__file__))) == os.path.abspath(package_root), lib.__file__
    spec = importlib.util.spec_from_file_location("param_grad_paths", os.path.join(ROOT, "tests", "test_param_grad_paths_gpu.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    dev = torch.device("cuda:0")
    cases = {}
    for part in (_op_cases, _glue_cases, _model_step):
        cases.update(part(T, lib, dev))
        print(f"[ops_trace] {part.__name__}: {len(cases)} cases so far", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(cases, f, indent=0, sort_keys=True)
    print(f"[ops_trace] {len(cases)} cases, {sum(len(c['calls']) for c in cases.values())} calls -> {path}")


def compare(a_path, b_path, out_path, commits):
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    diffs = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            diffs.append({"case": k, "what": "missing in " + ("first" if k not in a else "second")})
            continue
        for field in ("calls", "reported", "recorded", "sha256"):
            if a[k][field] != b[k][field]:
                diffs.append({"case": k, "what": field})
    res = {"commits": list(commits), "cases": len(a), "recorded_calls": sum(len(c["calls"]) for c in a.values()),
           "reported_names": sum(len(c["reported"]) + len(c["recorded"]) for c in a.values()),
           "hashed_tensors": sum(len(c["sha256"]) for c in a.values()), "identical": not diffs and a == b, "differences": diffs}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if res["identical"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--compare", nargs=3, metavar=("A", "B", "SUMMARY"))
    ap.add_argument("--commits", nargs=2, default=("", ""))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.commits))
    trace(a.out, a.package_root)
