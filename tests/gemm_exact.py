"""Host side of the exact GEMM tests (tests/test_gemm_exact_gpu.py, tests/test_gemm_exact_inputs_cpu.py): operands for which a GEMM has
ONE right answer whatever the summation order, the integer reference, the conditions under which that claim holds, guarded output
buffers and the comparator. Nothing here touches the GPU library at import time.

Why tolerance zero is legitimate. bf16 operands drawn from {-1, 0, +1} multiply exactly; every fp32 partial sum over any K range is an
integer of magnitude <= sum_k |a||b|. If that bound is <= 256 every partial sum is representable in bf16 (8 significand bits: all
integers up to 256, all multiples of 0.5 up to 128), so a bf16 split-K partial (policy key 1), the bf16 tile epilogue's read-out and the
final rounding lose nothing; alpha a power of two, an integer bias, ReLU / its derivative, a multiply by {-1, 0, 1} and `C +=` on an integer C
keep it that way. For fp32 outputs the bound is 2^24. `check_exactness_conditions` asserts all of it per case, so a case that stops being
exact fails as a CASE, not as a kernel."""
from dataclasses import dataclass
from functools import lru_cache

import torch

CANARY, UNWRITTEN = -320.0, -384.0       # both exact in bf16, both outside any result (|result| <= 256)
from valor_amd.lib import ACT_DERIV, ACT_NONE, ACT_RELU  # noqa: E402  (plain constants: the library is not loaded)


@dataclass(frozen=True)
class Case:
    """one valor_gemm call. `knobs`: tuple of (name, value) applied before the call -- variant, tr_asm, fast_epi, sched, nsched, key<k>,
    skinny_tile ("mt,ns"), skinny (per-call policy key 11). `family`: what valor_gemm_kernel_for must answer under those knobs."""
    name: str
    family: int
    M: int
    N: int
    K: int
    ta: bool = False
    tb: bool = False
    f32: bool = False                 # fp32 operands (dense integers in [-3, 3]); otherwise bf16 in {-1, 0, 1}
    out_f32: bool = False             # fp32 output of bf16 operands
    dense: bool = False               # bf16 operands in [-3, 3] (fp32 output only): sums far beyond what bf16 holds, so that a bf16 rounding
                                      # anywhere on the way to an fp32 result (a bf16 split-K partial, a bf16 tile pass) shows
    alpha: float = 1.0
    bias: bool = False
    act: int = ACT_NONE               # ACT_RELU, optionally | ACT_DERIV
    preact: bool = False              # second output: u, or relu'(u) under ACT_DERIV
    aux: str = ""                     # "deriv": dact_aux in {-1, 0, 1} with ACT_DERIV; "relu": dact_aux = a saved integer pre-activation
    acc: bool = False                 # C += onto an integer C0
    rowsum: str = ""                  # "" | "plain" | "acc"
    splitk: bool = False              # a workspace is offered
    split: bool = False               # ... and the slicing rule must actually cut K (asserted)
    wave128: bool = False             # family 3 on the four-wave kernel (asserted through valor_gemm_wave128_for)
    exact_ws: bool = False            # the workspace is a piece of exactly the bytes the slicing needs, cut from a guarded buffer
    ld_extra: int = 8
    knobs: tuple = ()
    seed: int = 1
    budget: int = 64

    @property
    def heavy(self):
        return self.aux == "relu"


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


@lru_cache(maxsize=64)
def _logical(M, N, K, seed, budget, dense):
    """A [M, K], B [N, K] as float64 (cached: many cases share a product)"""
    g = _gen(seed * 1000003 + 17)
    if dense:
        A = torch.randint(-3, 4, (M, K), generator=g).double()
        B = torch.randint(-3, 4, (N, K), generator=g).double()
        return A, B
    d = min(1.0, (budget / K) ** 0.5)

    def tern(rows):
        nz = torch.rand((rows, K), generator=g) < d
        sg = torch.randint(0, 2, (rows, K), generator=g) * 2 - 1
        return (nz * sg).double()
    return tern(M), tern(N)


def operands(M, N, K, ta, tb, seed, budget=64, dtype=torch.float32, dense=False):
    """A and B in the layout the call needs ([M, K], or [K, M] when ta; [N, K], or [K, N] when tb), contiguous, on the CPU. Entries in
    {-1, 0, +1} with nonzero density min(1, sqrt(budget / K)) -- about `budget` nonzero products per output element --, uniform signs;
    dense=True: integers in [-3, 3] (fp32-output / fp32-dtype cases only). The VALUES do not depend on the layout."""
    A, B = _logical(M, N, K, seed, budget, bool(dense))
    A = (A.t() if ta else A).contiguous().to(dtype)
    B = (B.t() if tb else B).contiguous().to(dtype)
    return A, B


def epilogue_inputs(case):
    """the integer side inputs of a case (float64, CPU): bias [N], aux [M, N], C0 [M, N], r0 [M]; None where the case has none"""
    g = _gen(case.seed * 7919 + 5)
    M, N = case.M, case.N
    bias = (torch.arange(N) % 61 - 30).double() if case.bias else None        # distinct neighbours: a column shift shows
    aux = None
    if case.aux == "deriv":
        aux = (torch.randint(0, 10, (M, N), generator=g).double() > 1.5) * (torch.randint(0, 2, (M, N), generator=g) * 2.0 - 1.0)
    elif case.aux == "relu":
        aux = torch.randint(-40, 41, (M, N), generator=g).double()
    C0 = torch.randint(-60, 61, (M, N), generator=g).double() if case.acc else None
    r0 = torch.randint(-60, 61, (M,), generator=g).double() if case.rowsum == "acc" else None
    return bias, aux, C0, r0


def reference(A, B, ta, tb, alpha=1.0, bias=None, act=ACT_NONE, want_preact=False, aux=None, C0=None, want_rowsum=False, r0=None):
    """epilogue_store of csrc/gemm_common.h in float64 on the CPU: v = alpha * acc + bias; the activation (skipped when an act' operand is
    given); the `preact` copy -- u, or act'(u) under ACT_DERIV --; the dact_aux multiply -- the saved value itself under ACT_DERIV,
    [aux > 0] for plain ReLU --; + C0. Returns (C, preact or None, row sums of op(A) (+ r0) or None)."""
    A, B = A.double(), B.double()
    opA = A.t() if ta else A
    opB = B.t() if tb else B
    v = alpha * (opA @ opB.t())
    if bias is not None:
        v = v + bias.double()[None, :]
    kind, deriv = act & 15, bool(act & ACT_DERIV)
    assert kind in (ACT_NONE, ACT_RELU), "only the exact epilogues have a reference here"
    pre = v
    if (kind != ACT_NONE or (deriv and want_preact)) and aux is None:
        if want_preact and deriv:
            pre = (v > 0).double() if kind == ACT_RELU else torch.ones_like(v)
        if kind == ACT_RELU:
            v = torch.clamp_min(v, 0.0)
    if aux is not None:
        a = aux.double()
        v = v * (a if deriv else ((a > 0).double() if kind == ACT_RELU else torch.ones_like(a)))
    if C0 is not None:
        v = v + C0.double()
    rs = None
    if want_rowsum:
        rs = opA.sum(dim=1)
        if r0 is not None:
            rs = rs + r0.double()
    return v, (pre if want_preact else None), rs


def case_reference(case):
    """(A, B) in the case's layout and dtype-agnostic float64, the side inputs, and the reference outputs"""
    A, B = operands(case.M, case.N, case.K, case.ta, case.tb, case.seed, case.budget, torch.float64, dense=case.f32 or case.dense)
    bias, aux, C0, r0 = epilogue_inputs(case)
    C, pre, rs = reference(A, B, case.ta, case.tb, case.alpha, bias, case.act, case.preact, aux, C0, bool(case.rowsum), r0)
    return dict(A=A, B=B, bias=bias, aux=aux, C0=C0, r0=r0, C=C, preact=pre, rowsum=rs)


def _no_duplicate_rows(x):
    return torch.unique(x, dim=0).shape[0] == x.shape[0]


def check_exactness_conditions(case, ref=None):
    """the conditions under which the case has exactly one right answer, and under which passing it means something"""
    ref = ref or case_reference(case)
    A, B = ref["A"], ref["B"]
    opA = (A.t() if case.ta else A).abs()
    opB = (B.t() if case.tb else B).abs()
    absprod = float((opA @ opB.t()).max())                     # bounds EVERY partial sum of every K range
    limit = 2.0 ** 24 if (case.f32 or case.out_f32) else 256.0
    assert case.alpha in (0.5, 1.0, 2.0), "alpha must be a power of two"
    assert not case.dense or case.out_f32, "the dense operands are for fp32 results"
    assert float(torch.maximum(opA.max(), opB.max())) <= (3.0 if (case.f32 or case.dense) else 1.0), "operands of bf16 results are drawn from {-1, 0, 1}"
    assert absprod <= limit, f"{case.name}: partial sums up to {absprod} are not exact (limit {limit})"
    bound = absprod * abs(case.alpha)
    if ref["bias"] is not None:
        bound += float(ref["bias"].abs().max())
    if case.aux == "deriv":
        assert float(ref["aux"].abs().max()) <= 1.0
        bound *= float(ref["aux"].abs().max())
    if ref["C0"] is not None:
        bound += float(ref["C0"].abs().max())
    # alpha = 0.5 halves the integers: multiples of 0.5 are exact in bf16 below 128 only
    lim_out = limit / 2 if case.alpha == 0.5 and limit == 256.0 else limit
    assert bound <= lim_out, f"{case.name}: |result| can reach {bound} > {lim_out}"
    outs = [ref["C"]] + ([ref["preact"]] if ref["preact"] is not None else [])
    for o in outs:
        assert float(o.abs().max()) <= lim_out and bool((o * 2 == torch.round(o * 2)).all())
        if case.alpha != 0.5:
            assert bool((o == torch.round(o)).all())
        if limit == 256.0:           # (an fp32 result of the dense operands may be any integer: there the canaries only guard what lies OUTSIDE the view)
            assert not bool((o == CANARY).any()) and not bool((o == UNWRITTEN).any())
    if ref["rowsum"] is not None:
        assert float(ref["rowsum"].abs().max()) <= limit, f"{case.name}: |row sums| reach {float(ref['rowsum'].abs().max())}"
        if min(case.K, 64) >= 16:                                     # (an 8-term sum of +-1 repeats among 8 rows: nothing to tell apart)
            assert float((ref["rowsum"] != 0).double().mean()) > 0.5
    # not vacuous. The linear part u = alpha * acc + bias is what a dropped K-tile, a misplaced fragment or a permutation changes: more than
    # half of it is nonzero. ReLU (or relu'(aux)) zeroes about half of any zero-mean integer result by construction, so the final output of
    # those cases is asked for a quarter; every other case for more than half, as the linear part.
    u = case.alpha * ((A.t() if case.ta else A) @ (B.t() if case.tb else B).t())
    if ref["bias"] is not None:
        u = u + ref["bias"][None, :]
    # (an 8 x 8 x 8 product is in the table for its bounds: eight +-1 terms cannot fill a tile with distinct rows)
    if min(case.M, case.N, case.K) >= 16:
        assert float((u != 0).double().mean()) > 0.5, f"{case.name}: the product is mostly zero"
        relu_like = (case.act & 15) == ACT_RELU and (case.aux != "deriv")
        frac = float((ref["C"] != 0).double().mean())
        assert frac > (0.25 if relu_like else 0.5), f"{case.name}: only {frac:.2f} of the output is nonzero"
        # no two rows and no two columns of the result are equal: a row or column permutation cannot pass. (Behind a ReLU the columns
        # whose bias is -30 are all zero and so equal; there the linear part, which the ReLU is applied to element by element, is asked.)
        distinct = u if relu_like else ref["C"]
        assert _no_duplicate_rows(distinct), f"{case.name}: duplicate rows in the reference"
        assert _no_duplicate_rows(distinct.t().contiguous()), f"{case.name}: duplicate columns in the reference"
    return dict(absprod=absprod, bound=bound, nonzero=float((ref["C"] != 0).double().mean()))


def guarded(M, N, dtype, dev, ld_extra, rows=2, prefill=True):
    """(buf, view): a buffer of M + 2 * rows rows with leading dimension N + ld_extra filled with the canary -320, and its [M, N] view that
    starts `rows` rows in. prefill: the view holds a second canary, -384 (a call that does not accumulate must overwrite every element).
    N = None: a 1-D vector of M elements with 8 * rows guard elements on either side."""
    if N is None:
        g = 8 * rows
        buf = torch.full((M + 2 * g,), CANARY, dtype=dtype, device=dev)
        view = buf[g:g + M]
    else:
        buf = torch.full((M + 2 * rows, N + ld_extra), CANARY, dtype=dtype, device=dev)
        view = buf[rows:rows + M, :N]
    if prefill:
        view.fill_(UNWRITTEN)
    return buf, view


def _view_mask(buf, view):
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    off = view.storage_offset() - buf.storage_offset()
    if buf.dim() == 1:
        mask[off:off + view.shape[0]] = True
    else:
        r0, c0 = divmod(off, buf.stride(0))
        mask[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = True
    return mask


class Mismatch(AssertionError):
    def __init__(self, report):
        self.report = report
        super().__init__(format_report(report))


def diagnose(got, want, buf=None, view=None, max_list=8):
    """what is wrong with `got` ([M, N] or [M]) against `want`, and with the guard elements of `buf` around `view`; None if nothing is"""
    got = got.detach().cpu().double()
    want = want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    one_d = got.dim() == 1
    g2, w2 = (got[:, None], want[:, None]) if one_d else (got, want)
    bad = ~(g2 == w2)                                   # value comparison: -0 == +0, NaN equals nothing
    rep = dict(count=int(bad.sum()), total=bad.numel(), nan=int(torch.isnan(g2).sum()), unwritten=int((g2 == UNWRITTEN).sum()),
               first=[], blocks16=[], tiles128=[], tiles256=[], rows=[], cols=[], row_alias=[], col_alias=[], guard=[])
    if buf is not None:
        b = buf.detach().cpu().double()
        hit = (~(b == CANARY)) & ~_view_mask(buf, view)
        rep["guard"] = [tuple(int(i) for i in ix) + (float(b[tuple(ix)]),) for ix in hit.nonzero()[:max_list]]
        rep["guard_count"] = int(hit.sum())
    if rep["count"]:
        idx = bad.nonzero()
        rep["first"] = [(int(m), int(n), float(g2[m, n]), float(w2[m, n])) for m, n in idx[:max_list]]
        for key, t in (("blocks16", 16), ("tiles128", 128), ("tiles256", 256)):
            rep[key] = sorted({(int(m), int(n)) for m, n in torch.unique(idx // t, dim=0)})
        rep["rows"] = sorted(int(m) for m in torch.unique(idx[:, 0]))
        rep["cols"] = sorted(int(n) for n in torch.unique(idx[:, 1]))
        # do the wrong values of a row (column) equal ANOTHER row (column) of the reference at the same places? -> a swap / misplaced fragment
        for m in rep["rows"][:max_list]:
            c = bad[m].nonzero()[:, 0]
            src = (w2[:, c] == g2[m, c][None, :]).all(dim=1).nonzero()[:, 0]
            rep["row_alias"] += [(m, int(s)) for s in src[:2] if int(s) != m]
        for n in rep["cols"][:max_list]:
            r = bad[:, n].nonzero()[:, 0]
            src = (w2[r, :] == g2[r, n][:, None]).all(dim=0).nonzero()[:, 0]
            rep["col_alias"] += [(n, int(s)) for s in src[:2] if int(s) != n]
    return rep if (rep["count"] or rep["guard"]) else None


def format_report(rep):
    lines = [f"{rep['count']} of {rep['total']} elements wrong ({rep['nan']} NaN, {rep['unwritten']} never written)"]
    if rep["first"]:
        lines.append("first (m, n, got, want): " + ", ".join(str(t) for t in rep["first"]))
        lines.append(f"16x16 blocks: {rep['blocks16'][:24]}{' ...' if len(rep['blocks16']) > 24 else ''}")
        lines.append(f"128-tiles: {rep['tiles128'][:24]}  256-tiles: {rep['tiles256'][:24]}")
        if rep["row_alias"]:
            lines.append(f"wrong rows hold the reference's rows (row, source): {rep['row_alias']}")
        if rep["col_alias"]:
            lines.append(f"wrong columns hold the reference's columns (column, source): {rep['col_alias']}")
    if rep["guard"]:
        lines.append(f"{rep.get('guard_count')} guard elements overwritten, first (index..., value): {rep['guard']}")
    return "\n".join(lines)


def compare(got, want, buf=None, view=None):
    """element for element at tolerance zero, every guard element of `buf` outside `view` still -320; raises Mismatch (an AssertionError whose
    .report says how many, where -- 16 x 16 blocks, 128- and 256-tiles -- and whether the wrong values are another row / column of the
    reference)"""
    rep = diagnose(got, want, buf, view)
    if rep is not None:
        raise Mismatch(rep)
