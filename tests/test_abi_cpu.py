"""CPU: the C-ABI library loads and exports exactly the symbols include/valor_hip.h declares, every kernel file is compiled against
that header, the ctypes table of valor_amd/lib.py matches it by argument type, struct layout and constant value, a C translation unit
including the header compiles, and the product refuses to run without a GPU (no CPU fallback)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "valor_hip.h")
CSRC = os.path.join(ROOT, "valor_amd", "csrc")


def _decls():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(valor_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
        out[m.group(1)] = [] if args == ["void"] else args
    return out


def test_library_exports_every_header_symbol():
    from valor_amd import lib
    lib.load()
    so = ctypes.CDLL(lib.LIB_PATH)
    decls = _decls()
    assert len(decls) >= 35
    for name in decls:
        assert hasattr(so, name), f"{name} declared in include/valor_hip.h but not exported"
    assert set(decls) == set(lib.SIGNATURES), set(decls) ^ set(lib.SIGNATURES)
    assert so.valor_adamw_chunk() == 1024 and so.valor_ln_part_blocks() > 0


C_SCALARS = ("int", "int64_t", "uint64_t", "float", "double")


def _c_class(param):
    """class of one parameter of a prototype: "pointer" or one of C_SCALARS; anything else is an error, not a guess"""
    if "*" in param:
        return "pointer"
    words = [w for w in param.split() if w != "const"]
    assert len(words) == 2 and words[0] in C_SCALARS, f"unrecognised C parameter {param!r}"
    return words[0]


def _ctypes_class(t):
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "pointer"
    # c_int32 / c_long alias c_int / c_int64 on this ABI: compare the classes, not the spellings
    known = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t", ctypes.c_float: "float", ctypes.c_double: "double"}
    assert t in known, f"unrecognised ctypes argument {t!r}"
    return known[t]


def test_signatures_match_header_by_type():
    """every argument of every entry of lib.SIGNATURES has the class of the header's parameter at that position: an int64_t stride bound
    as c_int, or a float bound as c_int, has the right COUNT and the wrong calling convention"""
    from valor_amd import lib
    decls = _decls()
    assert set(decls) == set(lib.SIGNATURES), set(decls) ^ set(lib.SIGNATURES)
    for name, params in decls.items():
        want = [_c_class(a) for a in params]
        got = [_ctypes_class(t) for t in lib.SIGNATURES[name]]
        assert got == want, (name, [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g] or (len(want), len(got)))


# public struct -> its ctypes mirror (valor_gemm_pending is opaque: its size is lib.GEMM_PENDING_BYTES)
STRUCTS = dict(valor_gemm_policy="GemmPolicy", valor_xattn_seg="XattnSeg", valor_reward_tables="RewardTables",
               valor_capeval_tables="CapevalTables", valor_capeval_summary="CapevalSummary")
INT_MACROS = ("VALOR_DT_BF16", "VALOR_DT_F32", "VALOR_ACT_NONE", "VALOR_ACT_GELU_ERF", "VALOR_ACT_QUICK_GELU", "VALOR_ACT_RELU",
              "VALOR_ACT_TANH", "VALOR_ACT_DERIV", "VALOR_STATS_FIELDS", "VALOR_METER_FIELDS", "VALOR_METER_MAX_SRC")


def _struct_fields(name):
    """member names of `typedef struct name { ... } name;` as the header spells them"""
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        for d in decl.split(","):
            m = re.search(r"(\w+)\s*(?:\[\d+\])?\s*$", d)
            if m:
                out.append(m.group(1))
    return out


def test_struct_layouts_and_constants_match_header(tmp_path):
    """gcc is the judge of the header: a C program prints sizeof, and offsetof / sizeof of every member, of every public struct and the
    value of every public macro, and the ctypes classes and constants of valor_amd/lib.py must say the same"""
    from valor_amd import lib
    lines = []
    for cname, pyname in STRUCTS.items():
        fields = _struct_fields(cname)
        assert fields == [f[0] for f in getattr(lib, pyname)._fields_], (cname, fields)
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu:%zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f in fields]
    assert _struct_fields("valor_gemm_pending") == ["opaque"]
    lines.append('printf("valor_gemm_pending %zu\\n", sizeof(valor_gemm_pending));')
    lines += [f'printf("{m} %d\\n", (int)({m}));' for m in INT_MACROS]
    lines.append('printf("VALOR_TRIE_FLOOR %a\\n", (double)(VALOR_TRIE_FLOOR));')
    c = tmp_path / "layout.c"
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "valor_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in r.stdout.splitlines())
    assert len(got) == len(lines)

    for cname, pyname in STRUCTS.items():
        cls = getattr(lib, pyname)
        assert int(got[cname]) == ctypes.sizeof(cls), (cname, got[cname], ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            # offset AND size: a member that shrinks in front of alignment padding moves nothing else
            assert got[f"{cname}.{f}"] == f"{getattr(cls, f).offset}:{getattr(cls, f).size}", (cname, f, got[f"{cname}.{f}"], getattr(cls, f))
    assert int(got["valor_gemm_pending"]) == lib.GEMM_PENDING_BYTES
    want = dict(VALOR_DT_BF16=lib.DT_BF16, VALOR_DT_F32=lib.DT_F32, VALOR_ACT_NONE=lib.ACT_NONE, VALOR_ACT_GELU_ERF=lib.ACT_GELU_ERF,
                VALOR_ACT_QUICK_GELU=lib.ACT_QUICK_GELU, VALOR_ACT_RELU=lib.ACT_RELU, VALOR_ACT_TANH=lib.ACT_TANH, VALOR_ACT_DERIV=lib.ACT_DERIV,
                VALOR_STATS_FIELDS=len(lib.STATS_FIELDS), VALOR_METER_FIELDS=len(lib.METER_FIELDS), VALOR_METER_MAX_SRC=lib.METER_MAX_SRC)
    assert set(want) == set(INT_MACROS)
    for m, v in want.items():
        assert int(got[m]) == v, (m, got[m], v)
    assert float.fromhex(got["VALOR_TRIE_FLOOR"]) == lib.TRIE_FLOOR


def test_library_exports_exactly_the_header():
    """the dynamic symbol table of the built library: every valor_* it defines is declared in the header, and the reverse"""
    from valor_amd import lib
    r = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("valor_")}
    assert exported == set(_decls()), exported ^ set(_decls())


def _quoted_includes(path):
    return [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M)]


def _without_stamp_blocks(text):
    """drop the `#if... *STAMP*` ... `#endif` blocks: the profiling builds' *_read_stamps entries are not part of the ABI"""
    out, skip_depth, depth = [], None, 0
    for line in text.splitlines():
        d = line.strip()
        if re.match(r"#\s*if", d):
            depth += 1
            if skip_depth is None and "STAMP" in d:
                skip_depth = depth
        if skip_depth is None:
            out.append(line)
        if re.match(r"#\s*endif", d):
            if skip_depth == depth:
                skip_depth = None
            depth -= 1
    assert depth == 0
    return "\n".join(out)


def test_every_kernel_file_is_compiled_against_the_header():
    """the quoted #include graph of every csrc/*.hip reaches include/valor_hip.h, so the compiler compares each extern "C" definition
    with its prototype; and no file declares a valor_* entry point itself: outside the stamp builds only definitions remain"""
    hips = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert len(hips) >= 35
    for f in hips:
        seen, todo = set(), [os.path.join(CSRC, f)]
        while todo:
            p = todo.pop()
            if p not in seen:
                seen.add(p)
                todo += _quoted_includes(p)
        assert os.path.normpath(HDR) in seen, f"{f} never includes include/valor_hip.h"
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            text = _without_stamp_blocks(re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(CSRC, f)).read(), flags=re.S))
            redecl = re.findall(r'extern\s+"C"[^;{}()]*\b(valor_\w+)\s*\([^;{}]*\)\s*;', text)
            assert not redecl, (f, redecl)


def test_header_is_plain_c(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "valor_hip.h"\nint (*fp)(void) = valor_adamw_chunk;\nint main(void){ return fp == 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_validation_without_gpu():
    """entry points validate arguments before touching the device (callable on a CPU-only host)."""
    from valor_amd import lib
    so = lib.load()
    assert so.valor_gemm(None, 0, 0, 0, 4, 4, 8, None, 8, None, 8, None, 4, None, 0, None, None, 0, 1.0, 0, 0, None, 0, None, 0) == -1
    assert so.valor_gemm(None, 0, 0, 0, 0, 4, 8, None, 8, None, 8, None, 4, None, 0, None, None, 0, 1.0, 0, 0, None, 0, None, 0) == 0   # M = 0: no-op
    assert so.valor_bdrln_fwd(None, 0, None, None, None, None, None, None, None, None, None, 4, 768, 1e-5, 0.0, 0, 0, None, 0, None) == -1
    # round-4 entries: the native reducer, the smoothed cross-entropy, the one-launch cross-attention
    import ctypes
    assert so.valor_reducer_unique_id(None) == -1 and so.valor_reducer_destroy(None) == 0
    assert so.valor_reducer_launch_bucket(None, 0, None, 0) == -1 and so.valor_reducer_wait(None, None) == -1
    h = ctypes.c_void_p()
    assert so.valor_reducer_create(ctypes.byref(h), None, 0, 1, 0, None, None, None, 1, 0) == -1
    buf = (ctypes.c_float * 64)()
    lab = (ctypes.c_int64 * 4)()
    assert so.valor_xent_smooth_fwd(None, 1, buf, lab, buf, buf, 4, 16, 16, 1.5) == -1            # smoothing outside [0, 1)
    assert so.valor_xent_smooth_bwd(None, 1, buf, lab, buf, None, 1.0, 4, 1, 16, 0.1) == -1       # smoothing needs V > 1
    assert so.valor_xent_smooth_fwd(None, 1, buf, lab, buf, buf, 0, 16, 16, 0.1) == 0             # no rows: no-op
    assert so.valor_cross_attn_fwd_fused(None, 0, None, 1, buf, buf, 1, 128, 1, 0, 64, 0, 64, 0.125, 0.0, None) == -1      # no segments
    assert so.valor_cross_attn_bwd_fused(None, 0, None, 3, buf, buf, buf, buf, 1, 128, 1, 0, 64, 0, 64, 0, 64, 0, 64, 0.125, 0.0, None) == -1


def test_adamw_argument_validation_without_gpu():
    """valor_adamw / valor_adamw_counted / valor_grad_norm_clip refuse bad sizes and group counts before any launch; n = 0 is a no-op"""
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    lr = (ctypes.c_float * 17)(*([1e-3] * 17))
    wd = (ctypes.c_float * 17)(*([0.0] * 17))

    def adamw(n, ngroups, dtype=0):
        return so.valor_adamw(None, dtype, p, p, p, p, p, p, n, lr, wd, ngroups, 0.9, 0.98, 1e-6, 1, 1, None, 1)

    def counted(n, ngroups, dtype=0, ntensors=1, chunk_bc=p):
        return so.valor_adamw_counted(None, dtype, p, p, p, p, p, p, p, p, ntensors, chunk_bc, n, lr, wd, ngroups, 0.9, 0.98, 1e-6, 1, None, 1)

    for f in (adamw, counted):
        assert f(1000, 10) == -1 and f(2048 + 1, 10) == -1            # n % 1024 != 0
        assert f(2048, 0) == -1 and f(2048, 17) == -1                 # ngroups outside 1..16
        assert f(2048, 10, dtype=7) == -1                             # unknown dtype
        assert f(0, 10) == 0 and f(0, 0) == 0                         # nothing to update: no-op
    assert counted(2048, 10, ntensors=0) == -1 and counted(2048, 10, chunk_bc=None) == -1
    assert so.valor_grad_norm_clip(None, 0, p, p, 1000, 1.0, 5.0, p, p, p) == -1
    assert so.valor_grad_norm_clip(None, 0, p, p, 0, 1.0, 5.0, p, p, p) == -1


def test_engine_refuses_grad_norm_the_fused_clip_would_misread():
    """the reference clips unless grad_norm == -1; the fused clip treats max_norm <= 0 as "off", so 0 / negative values are refused"""
    from types import SimpleNamespace
    from valor_amd.engine import TrainEngine
    for bad in (0.0, -2.0, -0.5):
        with pytest.raises(ValueError, match="grad_norm"):
            TrainEngine(None, SimpleNamespace(grad_norm=bad))


def test_per_call_gemm_policy_without_touching_process_state():
    """valor_gemm_policy (include/valor_hip.h): the kernel-family choice of ONE call, -1 = the process default. The family query is host
    logic, so the contract is checkable without a GPU: a policy changes the answer for its call only, the process defaults stay."""
    import ctypes
    from valor_amd import lib
    so = lib.load()
    assert ctypes.sizeof(lib.GemmPolicy) == 17 * 4
    M, N, K = 100864, 3072, 768                                    # ViT fc1 forward: family 4 under the default policy
    base = so.valor_gemm_kernel_for(0, 0, 0, M, N, K, 0)
    assert base == 4 and so.valor_gemm_kernel_for_tuned(None, 0, 0, 0, M, N, K, 0) == base
    never = lib.GemmPolicy.make(narrow=0)
    assert so.valor_gemm_kernel_for_tuned(ctypes.addressof(never), 0, 0, 0, M, N, K, 0) == 3          # the 256 x 256 kernel instead
    small = lib.GemmPolicy.make(variant=1)
    assert so.valor_gemm_kernel_for_tuned(ctypes.addressof(small), 0, 0, 0, M, N, K, 0) == 1          # the 128 x 128 kernel pinned
    assert so.valor_gemm_kernel_for(0, 0, 0, M, N, K, 0) == base                                       # nothing global moved
    assert so.valor_gemm_set_policy(8, -1) == 1000 and so.valor_gemm_set_variant(-1) == 4
    # argument validation happens under a policy too
    assert so.valor_gemm_tuned(ctypes.addressof(never), None, 0, 0, 0, 4, 4, 8, None, 8, None, 8, None, 4, None, 0, None, None, 0, 1.0, 0, 0, None, 0,
                               None, 0) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_no_cpu_fallback():
    from valor_amd import kernels as K, lib
    a = torch.zeros(8, 8)
    with pytest.raises(lib.ValorHipError):
        K.gemm(a, a)


def test_integration_snippets_match_header(tmp_path):
    """the C++ binding block compiles against include/valor_hip.h (stub torch headers, -fsyntax-only:
    the compiler checks arity and argument types of every valor_* call) and the ctypes block's argtypes equal the loader's."""
    from valor_amd import lib
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    cpp = re.findall(r"```cpp\n(.*?)```", doc, flags=re.S)
    assert cpp and "valor_bdrln_fwd" in cpp[0]
    src = tmp_path / "snippet.cpp"
    src.write_text(cpp[0])
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "stubs"),
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    py = [b for b in re.findall(r"```python\n(.*?)```", doc, flags=re.S) if "argtypes" in b]
    assert py
    m = re.search(r"lib\.(valor_\w+)\.argtypes = \[(.*?)\]", py[0])
    names = dict(vp=ctypes.c_void_p, i64=ctypes.c_int64, f=ctypes.c_float, u64=ctypes.c_uint64, i=ctypes.c_int)
    got = [names[t.strip()] for t in m.group(2).split(",")]
    assert got == lib.SIGNATURES[m.group(1)], (m.group(1), len(got), len(lib.SIGNATURES[m.group(1)]))
    call = re.search(r"lib\.valor_bdrln_fwd\((.*?)\)\s*#", py[0], flags=re.S) or re.search(r"rc = lib\.valor_bdrln_fwd\((.*?)\n\s*if rc", py[0], flags=re.S)
    assert call is not None
