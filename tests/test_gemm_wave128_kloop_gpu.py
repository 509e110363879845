"""K loop of the four-wave 128 x 128 wave-tile kernel (csrc/gemm8q.hip): the slot order -- eight slots of 16 MFMAs per K-tile, one
fragment read behind an MFMA, every k-half read at least two slots ahead of its first MFMA and waited for by a counted lgkmcnt one slot
after its last read, two barriers per K-tile, DMA look-ahead of two K-tiles -- against the eight-wave kernel of gemm8.hip bit for bit (C and the fused row sums) and against the fp32 product of the bf16
operands per 256 x 256 tile at the bounds of tests/test_gemm_wave128_gpu.py (2.5e-3 whole, 4e-3 worst tile). The kernel has one K-loop
order for this layout, so there is one arm.

K-tiles per workgroup. The launcher splits a wgrad with a workspace into sl = min(256 / tiles, nk / 6, 64) slices of per = ceil(nk / sl)
K-tiles, the trailing slices take what is left (nk = K / 64; csrc/gemm.hip, gemm_impl). For 1, 4 and 6 tiles (the three M, N below):
   K = 4096: nk 64, sl 10, per 7 -> nine slices of 7, the last of 1          K = 4160: nk 65, sl 10 -> the last of 2
   K = 5568: nk 87, sl 14, per 7 -> twelve of 7, one of 3, one EMPTY         K = 4288: nk 67, sl 11 -> nine of 7, one of 4, one EMPTY
   K = 5184: nk 81, sl 13, per 7 -> eleven of 7, one of 4, one EMPTY         K = 5696: nk 89, sl 14 -> twelve of 7, one of 5, one EMPTY
   K = 4416: nk 69, sl 11, per 7 -> nine of 7, one of 6, one EMPTY
   (2048, 1024, 4096): 32 tiles -> sl 8, per 8, every slice 8                without a workspace: 64 (even) and 65 (odd) in one workgroup
so every count from 0 to 8 is met -- the look-ahead of the slot order is two K-tiles deep, as is the prologue --, both buffer
parities at the exit, and slices shorter than the look-ahead whose remaining loads go through the zero-length descriptor.
Reference semantics: nn.Linear backward, model/bert.py:233-235,403-417."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL, TILE_TOL = 2.5e-3, 4e-3


def _mk(shape, seed, dev, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def _tile_errors(C, ref, tm=256, tn=256):
    d = (C.float() - ref)
    M, N = ref.shape
    Mp, Np = (M + tm - 1) // tm * tm, (N + tn - 1) // tn * tn
    pad = lambda x: torch.nn.functional.pad(x, (0, Np - N, 0, Mp - M))
    e2 = pad(d * d).view(Mp // tm, tm, Np // tn, tn).sum(dim=(1, 3))
    r2 = pad(ref * ref).view(Mp // tm, tm, Np // tn, tn).sum(dim=(1, 3))
    return float(torch.sqrt(e2.sum() / r2.sum())), float(torch.sqrt(e2 / r2.clamp_min(1e-20)).max())


@pytest.fixture
def w128(dev):
    """key 12 = 1 around the case (a process default: valor_gemm_policy keeps its 17 ints)"""
    from valor_amd import lib
    so = lib.load()
    old = so.valor_gemm_set_policy(12, 1)
    yield so
    so.valor_gemm_set_policy(12, old)


def _policy(**kw):
    from valor_amd import lib
    return lib.GemmPolicy.make(narrow=0, min_tiles=1, nt_min_tiles=1, **kw)


def _old(so, fn):
    """the same call on the eight-wave kernel"""
    o = so.valor_gemm_set_policy(12, 0)
    try:
        return fn()
    finally:
        so.valor_gemm_set_policy(12, o)


def _check_routing(so, M, N, K, pol):
    assert so.valor_gemm_wave128_for(0, 1, 1, M, N, K, 0) == 1
    assert so.valor_gemm_kernel_for_tuned(ctypes.addressof(pol), 0, 1, 1, M, N, K, 0) == 3
    assert _old(so, lambda: so.valor_gemm_wave128_for(0, 1, 1, M, N, K, 0)) == 0


_REF = {}


def _case(M, N, K, dev, bf16_partials, splitk):
    """dY [K, M], X [K, N], the fp32 product of the bf16 operands and the eight-wave kernel's C and row sums: once per case. Leading dimensions are multiples of 8 elements, so an M or N that is not is a column slice of a wider matrix."""
    from valor_amd import kernels as Kn, lib
    key = (M, N, K, bf16_partials, splitk)
    if key not in _REF:
        opk = (M, N, K)
        if opk not in _REF:
            A, B = _mk((K, (M + 7) // 8 * 8), 7 + M + K, dev)[:, :M], _mk((K, (N + 7) // 8 * 8), 11 + N + K, dev, 0.05)[:, :N]
            _REF[opk] = (A, B, A.float().t() @ B.float(), A.float().sum(0))
        A, B, ref, rs_ref = _REF[opk]
        so = lib.load()
        rs0 = torch.zeros((M,), dtype=torch.bfloat16, device=dev)
        C0 = _old(so, lambda: Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs0, splitk=splitk, policy=_policy(splitk_bf16=bf16_partials)))
        _REF[key] = (A, B, ref, rs_ref, C0, rs0)
    return _REF[key]


def _run(so, dev, M, N, K, bf16_partials, splitk=True):
    from valor_amd import kernels as Kn
    A, B, ref, rs_ref, C0, rs0 = _case(M, N, K, dev, bf16_partials, splitk)
    pol = _policy(splitk_bf16=bf16_partials)
    _check_routing(so, M, N, K, pol)
    rs = torch.zeros((M,), dtype=torch.bfloat16, device=dev)
    C = Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs, splitk=splitk, policy=pol)
    whole, worst = _tile_errors(C, ref)
    rs_err = float((rs.float() - rs_ref).norm() / rs_ref.norm())
    print(f"({M},{N},{K}) bf16 partials {bf16_partials} splitk {splitk}: whole {whole:.2e} worst tile {worst:.2e} row sums {rs_err:.2e}")
    assert whole < TOL and worst < TILE_TOL, (whole, worst)
    assert rs_err < TOL
    assert torch.equal(C, C0) and torch.equal(rs, rs0)


@pytest.mark.parametrize("bf16_partials", [1, 0])
@pytest.mark.parametrize("K", [4096, 4160, 5568, 5184, 4288, 5696, 4416])
@pytest.mark.parametrize("M,N", [(256, 256), (264, 280), (520, 392)])
def test_short_last_slices(w128, dev, M, N, K, bf16_partials):
    """slices of 7 K-tiles and a last one of 1 / 2 / 3 / 4 / 4 / 5 / 6, an empty slice where the module docstring says so"""
    _run(w128, dev, M, N, K, bf16_partials)


@pytest.mark.parametrize("bf16_partials", [1, 0])
def test_eight_ktiles_in_every_slice(w128, dev, bf16_partials):
    _run(w128, dev, 2048, 1024, 4096, bf16_partials)


@pytest.mark.parametrize("M,N,K", [(264, 280, 4096), (520, 392, 4160)])
def test_one_workgroup_per_tile(w128, dev, M, N, K):
    """no workspace offered: 64 and 65 K-tiles in one workgroup, the epilogue stores C and the row sums itself"""
    _run(w128, dev, M, N, K, 1, splitk=False)
