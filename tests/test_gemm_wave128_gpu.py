"""Family 3 on four waves of 128 x 128 outputs (csrc/gemm8q.hip, policy key 12): the 256 x 256 tile with one wave per SIMD. The kernel has
the k-slow x k-slow layout (weight gradients dW = dY^T . X) with the general fp32 epilogue; forced onto every family-3 problem of that
layout (key 12 = 1) it is compared bit for bit with the eight-wave kernel of gemm8.hip (same MFMA, same k order per accumulator and per
fused row sum) and per 256 x 256 tile with an fp32 torch.matmul of the bf16 operands, at the bounds of tests/test_gemm_wide_gpu.py.

Key 12 is a process default (valor_gemm_policy keeps its 17 ints), so the fixture sets and restores it; the other keys the cases need
(narrow kernel off, minimum-tile keys 1) go through the per-call policy.

K-tiles per workgroup. The launcher splits a wgrad into sl = min(256 / tiles, nk / 6, 64) slices of per = ceil(nk / sl) K-tiles, the
last slice takes what is left (nk = K / 64):
   K = 4096: nk 64, one tile  -> sl 10, per 7, last slice 1            K = 4160: nk 65 -> per 7, last slice 2
   K = 5184: nk 81 -> sl 13, per 7, last slice 3                        K = 5696: nk 89 -> sl 14, per 7, slice 12 has 5, slice 13 is EMPTY
   (2048, 1024, 4608): 32 tiles -> sl 8, per 9, every slice 9           without a workspace: 64 (even) and 65 (odd) K-tiles in one workgroup
so the prologue, the look-ahead past the last K-tile (zero-length descriptor), both buffer parities at the exit and a slice shorter than
the others are all met. Reference semantics: nn.Linear backward, model/bert.py:233-235,403-417, model/clip.py:176-192."""
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
    import ctypes
    assert so.valor_gemm_wave128_for(0, 1, 1, M, N, K, 0) == 1
    assert so.valor_gemm_kernel_for_tuned(ctypes.addressof(pol), 0, 1, 1, M, N, K, 0) == 3
    assert _old(so, lambda: so.valor_gemm_wave128_for(0, 1, 1, M, N, K, 0)) == 0


_REF = {}


def _operands(M, N, K, dev):
    """dY [K, M], X [K, N] and the fp32 product of the bf16 operands, computed once per shape. Leading dimensions are multiples of 8
    elements (16-byte rows), so an M or N that is not is a column slice of a wider matrix, as a fused QKV gradient is."""
    key = (M, N, K)
    if key not in _REF:
        A, B = _mk((K, (M + 7) // 8 * 8), 7 + M + K, dev)[:, :M], _mk((K, (N + 7) // 8 * 8), 11 + N + K, dev, 0.05)[:, :N]
        _REF[key] = (A, B, A.float().t() @ B.float())
    return _REF[key]


@pytest.mark.parametrize("K", [4096, 4160, 5184, 5696])
@pytest.mark.parametrize("M,N", [(256, 256), (264, 280), (300, 260), (520, 392)])
def test_wgrad_splitk_tails_and_ktile_counts(w128, dev, M, N, K):
    """split-K with bf16 and with fp32 partials (key 1), fused row sums, tails in M and N; 1 / 2 / 3 / 5 / 7 K-tiles per workgroup and an
    empty slice (see the module docstring)"""
    from valor_amd import kernels as Kn
    A, B, ref = _operands(M, N, K, dev)
    for bf16_partials in (1, 0):
        pol = _policy(splitk_bf16=bf16_partials)
        _check_routing(w128, M, N, K, pol)
        rs = torch.zeros((M,), dtype=torch.bfloat16, device=dev)
        C = Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs, policy=pol)
        whole, worst = _tile_errors(C, ref)
        print(f"({M},{N},{K}) bf16 partials {bf16_partials}: whole {whole:.2e} worst tile {worst:.2e}")
        assert whole < TOL and worst < TILE_TOL, (whole, worst)
        rs_ref = A.float().sum(0)
        assert float((rs.float() - rs_ref).norm() / rs_ref.norm()) < TOL
        rs0 = torch.zeros_like(rs)
        C0 = _old(w128, lambda: Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs0, policy=pol))
        assert torch.equal(C, C0) and torch.equal(rs, rs0)


@pytest.mark.parametrize("M,N,K,splitk", [(2048, 1024, 4608, True), (264, 280, 4096, False), (520, 392, 4160, False)])
def test_wgrad_long_slices_and_no_split(w128, dev, M, N, K, splitk):
    """9 K-tiles in every slice; 64 and 65 K-tiles in one workgroup when no workspace is offered (the epilogue stores C itself)"""
    from valor_amd import kernels as Kn
    A, B, ref = _operands(M, N, K, dev)
    pol = _policy()
    _check_routing(w128, M, N, K, pol)
    rs, rs0 = torch.zeros((M,), dtype=torch.bfloat16, device=dev), torch.zeros((M,), dtype=torch.bfloat16, device=dev)
    C = Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs, splitk=splitk, policy=pol)
    whole, worst = _tile_errors(C, ref)
    assert whole < TOL and worst < TILE_TOL, (whole, worst)
    C0 = _old(w128, lambda: Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs0, splitk=splitk, policy=pol))
    assert torch.equal(C, C0) and torch.equal(rs, rs0)


def test_wgrad_accumulate_and_fp32_out(w128, dev):
    """C += into an existing gradient buffer (row sums accumulated too) and fp32 output, with and without split-K"""
    from valor_amd import kernels as Kn
    M, N, K = 520, 392, 4160
    A, B, ref = _operands(M, N, K, dev)
    pol = _policy()
    _check_routing(w128, M, N, K, pol)
    for splitk in (True, False):
        base, rbase = _mk((M, N), 5, dev), _mk((M,), 6, dev)

        def run():
            out, rs = base.clone(), rbase.clone()
            Kn.gemm(A, B, trans_a=True, trans_b=True, out=out, accumulate=True, rowsum_out=rs, rowsum_accumulate=True, splitk=splitk, policy=pol)
            return out, rs
        out, rs = run()
        whole, worst = _tile_errors(out, ref + base.float())
        assert whole < 1.5 * TOL and worst < 1.5 * TILE_TOL, (whole, worst)
        rs_ref = A.float().sum(0) + rbase.float()
        assert float((rs.float() - rs_ref).norm() / rs_ref.norm()) < 1.5 * TOL
        out0, rs0 = _old(w128, run)
        assert torch.equal(out, out0) and torch.equal(rs, rs0)
        c32 = Kn.gemm(A, B, trans_a=True, trans_b=True, out_dtype=torch.float32, splitk=splitk, policy=pol)
        assert float((c32 - ref).norm() / ref.norm()) < 2e-5
        assert torch.equal(c32, _old(w128, lambda: Kn.gemm(A, B, trans_a=True, trans_b=True, out_dtype=torch.float32, splitk=splitk, policy=pol)))


def test_wgrad_deferred_group_reduction(w128, dev):
    """valor_gemm_deferred + valor_gemm_reduce_group with two products pending, as the backward pass queues its weight gradients"""
    shapes = ((520, 392, 4160), (264, 280, 4096))
    for M, N, K in shapes:
        assert w128.valor_gemm_wave128_for(0, 1, 1, M, N, K, 0) == 1 and w128.valor_gemm_kernel_for(0, 1, 1, M, N, K, 0) == 3

    def run():
        import ctypes
        from valor_amd import lib
        st = torch.cuda.current_stream(dev).cuda_stream
        piece = 32 << 20
        ws = torch.empty(len(shapes) * piece, dtype=torch.uint8, device=dev)
        blobs = (ctypes.c_char * (256 * len(shapes)))()
        outs = []
        for i, (M, N, K) in enumerate(shapes):
            A, B, _ = _operands(M, N, K, dev)
            out, rs = torch.zeros((M, N), dtype=torch.bfloat16, device=dev), torch.zeros((M,), dtype=torch.bfloat16, device=dev)
            blob = ctypes.addressof(blobs) + 256 * i
            lib.call("valor_gemm_deferred", st, 0, 1, 1, M, N, K, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), N, 0, 0, 0, 0, 0,
                     1.0, 1, 0, ws.data_ptr() + i * piece, piece, rs.data_ptr(), 1, blob)
            used = ctypes.c_int64(0)
            lib.call("valor_gemm_pending_bytes", blob, ctypes.cast(ctypes.byref(used), ctypes.c_void_p))
            assert 0 < used.value <= piece          # split along K: the partial tiles wait in the workspace piece
            outs.append((out, rs))
        lib.call("valor_gemm_reduce_group", st, 0, ctypes.cast(blobs, ctypes.c_void_p), len(shapes))
        torch.cuda.synchronize()
        return outs
    new, old = run(), _old(w128, run)
    for (M, N, K), (out, rs), (out0, rs0) in zip(shapes, new, old):
        ref = _operands(M, N, K, dev)[2]
        whole, worst = _tile_errors(out, ref)
        assert whole < TOL and worst < TILE_TOL, (whole, worst)
        assert torch.equal(out, out0) and torch.equal(rs, rs0)


def test_decoder_wgrad_shape(w128, dev):
    """the smallest real token count of the step: the decoder's fc1 weight gradient (768 x 3072 from 8832 tokens) under the default keys"""
    from valor_amd import kernels as Kn
    M, N, K = 768, 3072, 8832
    assert w128.valor_gemm_wave128_for(0, 1, 1, M, N, K, 0) == 1 and w128.valor_gemm_kernel_for(0, 1, 1, M, N, K, 0) == 3
    A, B, ref = _operands(M, N, K, dev)
    rs, rs0 = torch.zeros((M,), dtype=torch.bfloat16, device=dev), torch.zeros((M,), dtype=torch.bfloat16, device=dev)
    C = Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs)
    whole, worst = _tile_errors(C, ref)
    assert whole < TOL and worst < TILE_TOL, (whole, worst)
    assert torch.equal(C, _old(w128, lambda: Kn.gemm(A, B, trans_a=True, trans_b=True, rowsum_out=rs0))) and torch.equal(rs, rs0)


def test_repeated_launches_are_deterministic(w128, dev):
    """screen of the counted-vmcnt ring (its placement is argued from the counts in csrc/gemm8q.hip, not from this test): the same TT
    product 20 times into fresh outputs, the same bits every time"""
    from valor_amd import kernels as Kn
    for M, N, K in ((768, 3072, 8832), (520, 392, 4160)):
        A, B, _ = _operands(M, N, K, dev)
        c0 = Kn.gemm(A, B, trans_a=True, trans_b=True)
        assert torch.equal(c0, _old(w128, lambda: Kn.gemm(A, B, trans_a=True, trans_b=True)))
        for _ in range(20):
            assert torch.equal(Kn.gemm(A, B, trans_a=True, trans_b=True), c0)
