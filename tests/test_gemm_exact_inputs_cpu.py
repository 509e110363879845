"""The host side of the exact GEMM tests (tests/gemm_exact.py), without a GPU: the conditions that make tolerance zero legitimate hold for
every case tests/test_gemm_exact_gpu.py parametrizes (its table is imported, the two cannot drift); the reference agrees with torch.matmul
in float64 plus the epilogue written out longhand; and the comparator catches -- and locates -- the mistakes a Frobenius norm lets through.

The gap the GPU file closes, measured here on a 512 x 768 bf16 product with bias (K = 768, about 64 nonzero products per element;
`test_comparator_catches_what_a_norm_lets_through` asserts each figure stays below the 6e-3 of tests/test_kernel_variants_gpu.py and
tests/test_gemm_ln_gpu.py, so a norm test at that bound PASSES each of these wrong results):
  (a) one element off by 1:                                    8.3e-05 relative Frobenius error
  (b) two rows of one 16 x 16 block swapped:                   4.7e-03
  (d) bias shifted by one column on the last N % 8 columns:    3.7e-03   (N = 772: 768 itself has no tail)
The comparator fails all three at tolerance zero and names the element, the block and the columns."""
import pytest
import torch

import gemm_exact as GE
import test_gemm_exact_gpu as T
from gemm_exact import ACT_DERIV, ACT_RELU, Case

NORM_BOUND = 6e-3          # whole-tensor Frobenius bound of the norm tests


def _dedup(cases):
    """the conditions do not depend on knobs or paddings: one representative per (operands, epilogue)"""
    seen, out = set(), []
    for c in cases:
        key = (c.M, c.N, c.K, c.ta, c.tb, c.f32, c.out_f32, c.alpha, c.bias, c.act, c.preact, c.aux, c.acc, c.rowsum, c.seed, c.budget, c.dense)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_table_is_what_the_issue_asks_for():
    cs = T.CASES
    assert len({c.name for c in cs}) == len(cs)
    fams = {c.family for c in cs}
    assert fams == {0, 1, 2, 3, 4, 5}
    for fam in (0, 1, 2, 3):
        assert {(c.ta, c.tb) for c in cs if c.family == fam} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c.ta, c.tb) for c in cs if c.family == 4} == {(False, False), (False, True), (True, True)}
    assert {c.ld_extra for c in cs} == {8, 4, 3}
    f5 = [c for c in cs if c.family == 5 and T.runs_on_family(c) == 5]
    assert {c.K for c in f5} == {512, 768, 1024, 3072, 4096} and {c.M for c in f5} == {1, 2, 63, 64, 65, 193, 384} and {c.N for c in f5} == {16, 24, 1000}
    assert {dict(c.knobs)["skinny_tile"] for c in f5} == {"4,1", "4,2", "4,4", "8,1", "8,2", "auto"}
    for fam in (0, 1, 2, 3, 4):
        assert any(c.split for c in cs if c.family == fam) and any(c.exact_ws for c in cs if c.family == fam)
    assert any(c.split and c.wave128 for c in cs) and any(c.exact_ws and c.wave128 for c in cs)
    assert len(T.TWICE) == 2
    # every knob value the issue lists is set by some family-3 / family-4 case
    def values(fam, knob):
        return {dict(c.knobs).get(knob) for c in cs if c.family == fam} - {None}
    assert values(3, "sched") >= {0, 1} and values(3, "tr_asm") == {0, 1} and values(3, "fast_epi") == {0, 1, 2}
    assert values(3, "key4") == {0, 2, 1000} and values(3, "key5") == {0, 1} and values(3, "key12") >= {0, 1}
    assert values(4, "nsched") == {0, 1} and values(4, "key9") == {0, 1} and values(4, "key10") == {0, 1}
    # the tile epilogue and the general one are both reached in families 3 and 4, with every epilogue the tile path has
    cov = T.coverage()
    for fam in (3, 4):
        assert {k[4] for k in cov if k[0] == fam} >= {"tile", "general", "reduce"}
    assert {k[4] for k in cov if k[0] in (1, 2)} >= {"lean", "fused", "reduce"}


def test_conditions_hold_for_every_gpu_case():
    """exactness (partial sums, outputs, row sums inside what bf16 / fp32 hold exactly) and non-vacuity (mostly nonzero, no two rows or
    columns equal) for every case of the GPU file, deferred ones included"""
    worst = 0.0
    for c in _dedup(T.CASES + T.DEFERRED_CASES):
        info = GE.check_exactness_conditions(c)
        if not (c.f32 or c.out_f32):
            worst = max(worst, info["bound"])
    assert 0 < worst <= 256


def test_policy_sends_every_case_where_it_means_to_go():
    """valor_gemm_kernel_for* / valor_gemm_wave128_for are host logic: the family every case names is the one the library picks under the
    case's knobs, and the split-K expectation follows the slicing rule -- checked here so that no GPU time goes to a mistaken table"""
    from valor_amd import lib
    so = lib.load()
    before = T._snapshot(so)
    for c in T.CASES:
        k = T.Knobs(so)
        try:
            k.apply(c.knobs)
            assert T.family_of(so, c, k.policy) == c.family, c.name
            if not c.f32:
                assert bool(so.valor_gemm_wave128_for(0, int(c.ta), int(c.tb), c.M, c.N, c.K, int(c.heavy))) == c.wave128, c.name
            if c.splitk:
                fam = T.runs_on_family(c)
                ws = T.exact_ws_floats(c, fam)[1] * 4 if c.exact_ws else 256 << 20
                assert (T.expected_slices(c, fam, ws) > 1) == c.split, c.name
        finally:
            k.restore()
    assert T._snapshot(so) == before
    # the empty and the short trailing slice: 49 K-tiles in 8 slices of 7 leave the eighth empty, 50 leave it one K-tile
    c = next(c for c in T.CASES if c.split and c.K == 3136 and c.family == 3)
    s = T.expected_slices(c, 3, 256 << 20)
    assert s == 8 and (s - 1) * -(-49 // s) >= 49 and 0 < 50 - (s - 1) * -(-50 // s) < -(-50 // s)


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
def test_reference_against_matmul_and_a_longhand_epilogue(ta, tb):
    M, N, K = 37, 29, 50
    A, B = GE.operands(M, N, K, ta, tb, seed=3, dtype=torch.float64)
    assert A.shape == ((K, M) if ta else (M, K)) and B.shape == ((K, N) if tb else (N, K))
    assert set(A.unique().tolist()) <= {-1.0, 0.0, 1.0}
    acc = torch.matmul(A.t() if ta else A, B if tb else B.t())
    g = torch.Generator().manual_seed(9)
    bias = (torch.arange(N) % 61 - 30).double()
    C0 = torch.randint(-60, 61, (M, N), generator=g).double()
    aux = torch.randint(-3, 4, (M, N), generator=g).double()
    sav = torch.randint(-1, 2, (M, N), generator=g).double()
    r0 = torch.randint(-9, 10, (M,), generator=g).double()
    want = torch.empty(M, N, dtype=torch.float64)
    pre_u, pre_d, dm, dr = torch.empty_like(want), torch.empty_like(want), torch.empty_like(want), torch.empty_like(want)
    for m in range(M):
        for n in range(N):
            u = 0.5 * float(acc[m, n]) + float(bias[n])
            pre_u[m, n] = u
            pre_d[m, n] = 1.0 if u > 0 else 0.0
            want[m, n] = max(u, 0.0) + float(C0[m, n])
            dm[m, n] = 2.0 * float(acc[m, n]) * float(sav[m, n])
            dr[m, n] = float(acc[m, n]) * (1.0 if aux[m, n] > 0 else 0.0) + float(C0[m, n])
    C, pre, rs = GE.reference(A, B, ta, tb, alpha=0.5, bias=bias, act=ACT_RELU, want_preact=True, C0=C0, want_rowsum=True, r0=r0)
    assert torch.equal(C, want) and torch.equal(pre, pre_u)
    assert torch.equal(rs, (A.t() if ta else A).sum(dim=1) + r0)
    C, pre, _ = GE.reference(A, B, ta, tb, alpha=0.5, bias=bias, act=ACT_RELU | ACT_DERIV, want_preact=True, C0=C0)
    assert torch.equal(C, want) and torch.equal(pre, pre_d)
    C, pre, rs = GE.reference(A, B, ta, tb, alpha=2.0, act=ACT_RELU | ACT_DERIV, aux=sav)
    assert torch.equal(C, dm) and pre is None and rs is None
    C, _, _ = GE.reference(A, B, ta, tb, act=ACT_RELU, aux=aux, C0=C0)
    assert torch.equal(C, dr)
    Ad, Bd = GE.operands(M, N, K, ta, tb, seed=3, dtype=torch.float32, dense=True)
    assert float(Ad.abs().max()) == 3.0 and Ad.dtype == torch.float32
    C, _, _ = GE.reference(Ad, Bd, ta, tb)
    assert torch.equal(C, torch.matmul(Ad.double().t() if ta else Ad.double(), Bd.double() if tb else Bd.double().t()))


def _fro(got, want):
    return float((got - want).norm() / want.norm())


def _result(N):
    case = Case(name="mutations", family=1, M=512, N=N, K=768, bias=True)
    ref = GE.case_reference(case)
    GE.check_exactness_conditions(case, ref)
    return case, ref


def test_comparator_catches_what_a_norm_lets_through():
    case, ref = _result(768)
    want = ref["C"]
    buf, view = GE.guarded(512, 768, torch.bfloat16, "cpu", 8)
    view.copy_(want)
    GE.compare(view, want, buf, view)                                   # a correct result passes, -0 included
    neg0 = view.clone()
    neg0[want == 0] = -0.0
    GE.compare(neg0, want)
    # (a) one element off by 1
    got = want.clone()
    got[300, 517] += 1
    fa = _fro(got, want)
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(got, want)
    r = e.value.report
    assert r["count"] == 1 and r["first"][0][:2] == (300, 517) and r["blocks16"] == [(18, 32)] and r["tiles128"] == [(2, 4)] and r["tiles256"] == [(1, 2)]
    # (b) two rows of one 16 x 16 block swapped
    got = want.clone()
    got[130, 256:272], got[137, 256:272] = want[137, 256:272], want[130, 256:272]
    fb = _fro(got, want)
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(got, want)
    r = e.value.report
    assert r["blocks16"] == [(8, 16)] and r["rows"] == [130, 137] and set(r["row_alias"]) >= {(130, 137), (137, 130)}
    assert "(130, 137)" in str(e.value) and 16 < r["count"] <= 32
    # (c) one K-tile of 64 dropped from one 128 x 128 tile
    A, B = ref["A"], ref["B"]
    got = want.clone()
    got[256:384, 128:256] -= A[256:384, 192:256] @ B[128:256, 192:256].t()
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(got, want)
    r = e.value.report
    assert r["tiles128"] == [(2, 1)] and r["tiles256"] == [(1, 0)] and r["count"] > 128 * 128 // 2 and len(r["blocks16"]) == 64
    # (e) one guard element overwritten: behind the last column of a row, in a guard row, in front of the first row
    for ix in ((5, 768), (515, 3), (1, 775)):
        b2 = buf.clone()
        v2 = b2[2:514, :768]
        b2[ix] = 1.0
        with pytest.raises(GE.Mismatch) as e:
            GE.compare(v2, want, b2, v2)
        assert e.value.report["count"] == 0 and e.value.report["guard"] == [ix + (1.0,)]
    # (f) one interior element left at -384
    b2, v2 = GE.guarded(512, 768, torch.bfloat16, "cpu", 8)
    v2.copy_(want)
    v2[77, 400] = GE.UNWRITTEN
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(v2, want, b2, v2)
    r = e.value.report
    assert r["count"] == 1 and r["unwritten"] == 1 and r["first"][0] == (77, 400, GE.UNWRITTEN, float(want[77, 400])) and "never written" in str(e.value)
    # a NaN is a mismatch, never "equal"
    got = want.clone()
    got[0, 0] = float("nan")
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(got, want)
    assert e.value.report["nan"] == 1 and e.value.report["count"] == 1
    # (d) bias shifted by one column on the last N % 8 columns (N = 772)
    case, ref = _result(772)
    want = ref["C"]
    got = want.clone()
    got[:, 768:] += (ref["bias"][767:771] - ref["bias"][768:772])[None, :]
    fd = _fro(got, want)
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(got, want)
    r = e.value.report
    assert r["cols"] == [768, 769, 770, 771] and r["count"] == 4 * 512 and {b[1] for b in r["blocks16"]} == {48}
    # the figures of the module docstring: each of these wrong results is INSIDE the bound the norm tests apply
    print(f"frobenius: one element {fa:.3g}, swapped rows {fb:.3g}, shifted bias {fd:.3g}; norm tests allow {NORM_BOUND}")
    assert 0 < fa < NORM_BOUND and 0 < fb < NORM_BOUND and 0 < fd < NORM_BOUND


def test_row_sum_vectors_are_guarded_the_same_way():
    buf, view = GE.guarded(300, None, torch.float32, "cpu", 0)
    assert buf.numel() == 300 + 32 and bool((view == GE.UNWRITTEN).all()) and float(buf[15]) == GE.CANARY
    want = torch.arange(300).double() - 150
    view.copy_(want)
    GE.compare(view, want, buf, view)
    buf[316] = 0.0
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(view, want, buf, view)
    assert e.value.report["guard"] == [(316, 0.0)]
    view[7] += 1
    with pytest.raises(GE.Mismatch) as e:
        GE.compare(view, want)
    assert e.value.report["first"][0][:2] == (7, 0)
