"""Every attention kernel family WITH dropout against explicit fp64 attention that applies the keep mask restated on the host
(tests/dropout_ref.py: attn_drop_headkey / attn_drop_bits of csrc/attn_common.h, element index q * Skv + local key, head b * H + h).

Two kinds of assertion per case:
 (a) parity on random inputs -- o, dq, dk, dv within the tolerances the p = 0 tests of the same families use (fp32: 3e-6 forward,
     1e-5 backward; bf16: 1e-2 / 2e-2, relative L2);
 (b) single-bit probes -- structured inputs on which one output element depends on ONE mask bit, checked element by element: a
     flipped bit moves an element by 1 / ((1 - p) len) (times `scale` for dQ / dK), a quarter of that step for the smallest key
     range of the case is accepted. They show per family that forward and backward draw the same, documented mask (a relative
     L2 norm in bf16 cannot see a few wrong bits).
The family is chosen by dtype / shape / valor_attn_set_variant / valor_attn_set_res_pipeline, following the dispatch of attention.hip
(attn_fwd_launch / attn_bwd_launch), attention_res.hip (res_eligible, attn_res_bwd_launch) and attention_x.hip (x_nqs)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import dropout_ref as R
from test_attention_gpu import _rel
from test_cross_attn_fused_gpu import CASES as XCASES

pytestmark = pytest.mark.gpu
SCALE = 1.0 / math.sqrt(64)
RANGES3 = [(0, 330), (0, 200), (200, 130)]
DEVICE_BASE = 3 * 2 ** 40 + 12345


class Geo:
    """one launch geometry: B query batches of Sq rows, H heads, K / V batches of Skv rows; `ranges` (per query GROUP b // bmod) and
    `bmod` as valor_attn_fwd takes them; mask: None | 'causal' | 'pad' | 'causal+pad' (additive, -10000)"""

    def __init__(self, B, H, Sq, Skv, mask=None, ranges=None, bmod=0):
        self.B, self.H, self.Sq, self.Skv, self.bmod, self.E = B, H, Sq, Skv, bmod, H * 64
        self.Bkv = bmod if bmod > 0 else B
        self.self_attn = Sq == Skv and ranges is None and bmod == 0
        self.kvr = None
        if ranges is not None:
            self.kvr = torch.tensor([list(ranges[b // bmod]) for b in range(B)], dtype=torch.int32)
        self.min_len = Skv if ranges is None else min(ln for _, ln in ranges)
        self.mask = None
        if mask is not None:
            assert Sq == Skv
            g = torch.Generator().manual_seed(B * 100 + Sq)
            m = torch.ones((1, Sq, Sq))
            if "pad" in mask:       # at least half of the keys stay open
                lens = torch.randint(Sq // 2 + 1, Sq + 1, (B,), generator=g)
                lens[0] = Sq
                m = (torch.arange(Sq)[None, :] < lens[:, None]).float()[:, None, :].expand(B, Sq, Sq).clone()
            if "causal" in mask:
                m = torch.tril(m)
            self.mask = ((1.0 - m) * -10000.0).contiguous()
        self.tag = f"({B},{H},{Sq},{Skv})" + (f" {mask}" if mask else "") + (f" bmod={bmod}" if bmod else "") + (" ranged" if ranges else "")

    def on(self, dev):
        self.mask_dev = self.mask.to(dev) if self.mask is not None else None
        self.kvr_dev = self.kvr.to(dev) if self.kvr is not None else None
        return self


def _store(geo, dtype, qd, kd, vd):
    """dense q [B, Sq, E], k / v [Bkv, Skv, E] on the device -> strided views of fused buffers (row stride 3E / 2E) as the model keeps them"""
    E, dev = geo.E, qd.device
    if geo.self_attn:
        buf = torch.cat((qd, kd, vd), dim=-1).to(dtype)
        return buf[:, :, :E], buf[:, :, E:2 * E], buf[:, :, 2 * E:]
    qb = torch.zeros((geo.B, geo.Sq, 3 * E), dtype=dtype, device=dev)
    qb[:, :, :E] = qd
    kvb = torch.cat((kd, vd), dim=-1).to(dtype)
    return qb[:, :, :E], kvb[:, :, :E], kvb[:, :, E:]


@contextlib.contextmanager
def _family(variant=None, pipe=None):
    from valor_amd import lib
    so = lib.load()
    old_v, old_p = so.valor_attn_set_variant(-1), so.valor_attn_set_res_pipeline(-1)
    try:
        if variant is not None:
            so.valor_attn_set_variant(variant)
        if pipe is not None:
            so.valor_attn_set_res_pipeline(pipe)
        yield
    finally:
        so.valor_attn_set_variant(old_v)
        so.valor_attn_set_res_pipeline(old_p)


_KEEP = {}


def _keep(dev, geo, p, seed, offset, sel=None):
    """the host mask of the launch (offset = by-value offset + device base) as a bool tensor [B | len(sel), H, Sq, Skv] on the device"""
    key = (geo.B, geo.H, geo.Sq, geo.Skv, p, seed, offset, sel)
    if key not in _KEEP:
        if sel is None:
            m = R.attn_keep(seed, offset, geo.B, geo.H, geo.Sq, geo.Skv, p, kv_range=geo.kvr)
        else:
            heads = np.array([b * geo.H + h for b in sel for h in range(geo.H)])
            m = R.attn_keep_heads(seed, offset, heads, geo.Sq, geo.Skv, p).reshape(len(sel), geo.H, geo.Sq, geo.Skv)
        _KEEP[key] = torch.from_numpy(m).to(dev)
    return _KEEP[key]


def _run(geo, q, k, v, dout, p, seed, offset, fwd_only=False, unaligned=False, acc=False):
    """forward and backward of one family (whatever the dispatch picks under the current switches): (o, dq, dk, dv, known dK | dV buffer)"""
    from valor_amd import kernels as K
    kw = dict(mask=geo.mask_dev, kv_range=geo.kvr_dev, kv_bmod=geo.bmod, scale=SCALE, p_drop=p, seed=seed, offset=offset)
    o, lse = K.attn_fwd(q, k, v, geo.H, **kw)
    if fwd_only:
        return o, None, None, None, None
    E, grads, known = geo.E, {}, None
    if unaligned:       # one packed [B, S, 3E + 4] buffer: rows 8 bytes off a 16-byte pitch
        buf = torch.full((geo.B, geo.Sq, 3 * E + 4), float("nan"), dtype=q.dtype, device=q.device)
        grads = dict(dq=buf[:, :, :E], dk=buf[:, :, E:2 * E], dv=buf[:, :, 2 * E:3 * E])
    if acc:             # dK | dV added on top of a known buffer
        g = torch.Generator().manual_seed(77)
        known = (torch.randn((geo.Bkv, geo.Skv, 2 * E), generator=g) * 0.5).to(q.dtype).to(q.device)
        buf = known.clone()
        grads = dict(dk=buf[:, :, :E], dv=buf[:, :, E:])
    dq, dk, dv = K.attn_bwd(q, k, v, o, lse, dout, geo.H, accumulate_kv=acc, **grads, **kw)
    return o, dq, dk, dv, known


def _reference(geo, q, k, v, dout, keep, p, sel=None):
    if sel is not None:
        assert geo.self_attn and geo.mask is None
        ix = torch.tensor(sel, device=q.device)
        q, k, v, dout = q[ix], k[ix], v[ix], dout[ix]
    qd, kd, vd = (t.double().detach().requires_grad_(True) for t in (q, k, v))
    o = R.ref_attn_dropout(qd, kd, vd, geo.H, geo.mask_dev, geo.kvr, geo.bmod, SCALE, keep, p)
    (o * dout.double()).sum().backward()
    return o.detach(), qd.grad, kd.grad, vd.grad


def _pick(t, sel):
    return t if sel is None or t is None else t[torch.tensor(sel, device=t.device)]


def _parity(dev, geo, dtype, p=0.1, seed=7, offset=11, base=0, sel=None, **opts):
    geo.on(dev)
    g = torch.Generator().manual_seed(geo.B * 1000 + geo.Sq + geo.Skv)
    qd = (torch.randn((geo.B, geo.Sq, geo.E), generator=g) * 0.8).to(dev)
    kd = (torch.randn((geo.Bkv, geo.Skv, geo.E), generator=g) * 0.8).to(dev)
    vd = (torch.randn((geo.Bkv, geo.Skv, geo.E), generator=g) * 0.8).to(dev)
    dout = torch.randn((geo.B, geo.Sq, geo.E), generator=g).to(dtype).to(dev)
    q, k, v = _store(geo, dtype, qd, kd, vd)
    *got, known = _run(geo, q, k, v, dout, p, seed, offset, **opts)
    want = list(_reference(geo, q, k, v, dout, _keep(dev, geo, p, seed, offset + base, sel), p, sel))
    if known is not None:
        want[2] = want[2] + known[:, :, :geo.E].double()
        want[3] = want[3] + known[:, :, geo.E:].double()
    tol_f, tol_b = (3e-6, 1e-5) if dtype == torch.float32 else (1e-2, 2e-2)
    errs = {n: _rel(_pick(a, sel), b) for n, a, b in zip(("o", "dq", "dk", "dv"), got, want) if a is not None}
    print("PARITY", geo.tag, str(dtype)[6:], f"p={p}", {n: f"{e:.2e}" for n, e in errs.items()}, f"tol {tol_f:g}/{tol_b:g}")
    for n, e in errs.items():
        assert e < (tol_f if n == "o" else tol_b), (n, e)


def _onehot(n, c, dev):
    """[n, 64]: row r has a one in column r % 64 iff r // 64 == c"""
    r = torch.arange(n, device=dev)[:, None]
    return ((r // 64 == c) & (r % 64 == torch.arange(64, device=dev)[None, :])).float()


def _rows(t, nb, n, H):
    """[n, 64] or [64] -> [nb, n, H * 64]: the same 64 values in every head and batch"""
    return t.expand(n, 64).repeat(1, H)[None].expand(nb, n, H * 64).contiguous()


def _probe_inputs(geo, dev):
    """yields (name, outputs to check, q, k, v, dout) dense fp32 on the device -- see the module docstring and the issue's four probes"""
    B, Bkv, H, Sq, Skv = geo.B, geo.Bkv, geo.H, geo.Sq, geo.Skv
    ck, cq = (Skv + 63) // 64, (Sq + 63) // 64
    e0 = torch.zeros(64, device=dev)
    e0[0] = 1.0
    zq, zk = torch.zeros((B, Sq, geo.E), device=dev), torch.zeros((Bkv, Skv, geo.E), device=dev)
    ones_v, ones_do = _rows(e0, Bkv, Skv, H), _rows(e0, B, Sq, H)
    for c in range(max(ck, cq)):
        # q = 0: uniform probabilities. V one-hot per key of chunk c: o[b, q, h, d] = P keep / (1 - p) of key 64c + d;
        # dO one-hot per query of chunk c: dV[key, h, d] = sum over the batches sharing the K/V set of P keep / (1 - p) of query 64c + d
        yield f"fwd+dV chunk {c}", ("o", "dv"), zq, zk, _rows(_onehot(Skv, c, dev), Bkv, Skv, H), _rows(_onehot(Sq, c, dev), B, Sq, H)
    for c in range(ck):
        # K one-hot per key of chunk c, V = dO = e_0 (dP = 1): dQ[q, h, d] = scale dS[q, 64c + d]
        yield f"dS in dQ chunk {c}", ("dq",), zq, _rows(_onehot(Skv, c, dev), Bkv, Skv, H), ones_v, ones_do
    for c in range(cq):
        # Q one-hot per query of chunk c, K constant (a row's scores are constant): dK[key, h, d] = scale dS[64c + d, key]
        yield f"dS in dK chunk {c}", ("dk",), _rows(_onehot(Sq, c, dev), B, Sq, H), zk + 0.5, ones_v, ones_do


def _probes(dev, geo, dtype, p=0.1, seed=7, offset=11, base=0, sel=None, fwd_only=False, **opts):
    geo.on(dev)
    keep = _keep(dev, geo, p, seed, offset + base, sel)
    step = R.keep_scale(p) / geo.min_len
    tol = {"o": 0.25 * step, "dv": 0.25 * step, "dq": 0.25 * step * SCALE, "dk": 0.25 * step * SCALE}
    worst = {}
    for name, outs, qd, kd, vd, dod in _probe_inputs(geo, dev):
        if fwd_only and "o" not in outs:
            continue
        q, k, v = _store(geo, dtype, qd, kd, vd)
        dout = dod.to(dtype)
        got = dict(zip(("o", "dq", "dk", "dv"), _run(geo, q, k, v, dout, p, seed, offset, fwd_only=fwd_only, **opts)[:4]))
        want = dict(zip(("o", "dq", "dk", "dv"), _reference(geo, q, k, v, dout, keep, p, sel)))
        for n in outs:
            if got[n] is None:
                continue
            err = (_pick(got[n], sel).double() - want[n]).abs().max().item()
            worst[n] = max(worst.get(n, 0.0), err / tol[n])
            assert err < tol[n], (name, n, err, tol[n])
    print("PROBES", geo.tag, str(dtype)[6:], f"p={p}", "worst error / accepted:", {n: f"{e:.3f}" for n, e in worst.items()})


def _check(kind, *a, **kw):
    (_parity if kind == "parity" else _probes)(*a, **kw)


KINDS = pytest.mark.parametrize("kind", ["parity", "probes"])
STREAM_CASES = [
    (dict(B=2, H=3, Sq=70, Skv=130), 0.1),
    (dict(B=3, H=2, Sq=33, Skv=33, mask="causal+pad"), 0.1),
    (dict(B=6, H=2, Sq=32, Skv=330, ranges=RANGES3, bmod=2), 0.1),
    (dict(B=2, H=3, Sq=70, Skv=130), 0.25),
]
_ids = lambda c: Geo(**c[0]).tag.replace(" ", "-") + f"-p{c[1]}"     # noqa: E731


@KINDS
@pytest.mark.parametrize("case", STREAM_CASES, ids=_ids)
def test_streaming_fp32(dev, case, kind):
    """attn_fwd_kernel<float> / attn_bwd_dq_kernel<float> / attn_bwd_dkv_kernel<float> (attention.hip): fp32 never takes a fast path
    (attn_fwd_launch / attn_bwd_launch test ElemTraits<T>::DT == BF16). At 3e-6 / 1e-5 one wrong mask bit fails the parity."""
    _check(kind, dev, Geo(**case[0]), torch.float32, p=case[1])


@KINDS
@pytest.mark.parametrize("case", STREAM_CASES[:3], ids=_ids)
def test_streaming_bf16(dev, case, kind):
    """the same three kernels in bf16: valor_attn_set_variant(0) clears the resident (bit 0) and key-stationary (bit 1) fast paths"""
    with _family(variant=0):
        _check(kind, dev, Geo(**case[0]), torch.bfloat16, p=case[1])


@KINDS
@pytest.mark.parametrize("pipe", [0, 2])
@pytest.mark.parametrize("case", [dict(B=2, H=2, Sq=197, Skv=197), dict(B=2, H=2, Sq=129, Skv=129), dict(B=2, H=2, Sq=256, Skv=256),
                                  dict(B=3, H=2, Sq=100, Skv=100, mask="pad")], ids=lambda c: Geo(**c).tag.replace(" ", "-"))
def test_resident_forward_and_per_head_backward(dev, case, pipe, kind):
    """attn_res_fwd_kernel + attn_res_bwd_kernel (pipeline mode 0: 8 waves x 32-row blocks per (batch, head)) / attn_res_bwd16_kernel
    (mode 2: 16 waves x 16-row blocks): bf16, Sq == Skv <= 256, no kv_range / kv_bmod (res_eligible), 64 < S.
    The masked case uses a pad mask that leaves more than half of the keys open: with a causal mask at S = 100 the first rows hold
    probabilities of 1 and 1/2, whose bf16 rounding (2^-8 relative) is above a quarter of the 1 / (0.9 * 100) step."""
    with _family(pipe=pipe):
        _check(kind, dev, Geo(**case), torch.bfloat16)


@KINDS
@pytest.mark.parametrize("case", [dict(B=3, H=12, Sq=32, Skv=32, mask="causal"), dict(B=2, H=12, Sq=42, Skv=42, mask="pad"),
                                  dict(B=3, H=2, Sq=7, Skv=7), dict(B=2, H=2, Sq=64, Skv=64)], ids=lambda c: Geo(**c).tag.replace(" ", "-"))
def test_one_wave_backward(dev, case, kind):
    """attn_res_fwd_kernel + attn_res_bwd1_kernel (one wave per (batch, head), dQ and dK / dV in one launch): bf16 self-attention of
    S <= 64 rows (attn_res_bwd_launch: p.Skv <= 64)"""
    _check(kind, dev, Geo(**case), torch.bfloat16)


@KINDS
@pytest.mark.parametrize("pipe,unaligned", [(1, False), (3, False), (1, True)])
def test_persistent_backward(dev, pipe, unaligned, kind):
    """attn_res_bwd_pipe2_kernel (mode 1, every gradient row 16-byte aligned) / attn_res_bwd_pipe_kernel (mode 3, or mode 1 with the
    gradients in a packed view whose pitch is no multiple of 16 bytes): one workgroup per CU walks (batch, head) items, taken when
    B * H >= 2 x CUs and S > 160 -- 43 x 12 = 516 items of 197 rows on 256 CUs. fp64 on batches 0, 21 and 42."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert 43 * 12 >= 2 * cus, "the shape no longer reaches the persistent kernel on this device"
    with _family(pipe=pipe):
        _check(kind, dev, Geo(43, 12, 197, 197), torch.bfloat16, sel=(0, 21, 42), unaligned=unaligned)


@KINDS
@pytest.mark.parametrize("case,fwd_only", [(dict(B=2, H=2, Sq=42, Skv=330, bmod=2), False),
                                           (dict(B=6, H=2, Sq=16, Skv=330, ranges=RANGES3, bmod=2), False),
                                           (dict(B=6, H=2, Sq=32, Skv=330, ranges=RANGES3, bmod=2), True)],
                         ids=lambda c: Geo(**c).tag.replace(" ", "-") if isinstance(c, dict) else ("fwd" if c else "fwd+bwd"))
def test_key_stationary(dev, case, fwd_only, kind):
    """attn_x_fwd_kernel / attn_x_bwd_kernel (attention_x.hip): bf16, no additive mask, Skv >= 128 and (B / bmod) * ceil(Sq / 16) query
    sub-tiles <= 8 forward, <= 4 backward (x_nqs): 3, 3 and 6 here -- the last one forward only (its backward is the streaming pair).
    The grouped cases draw with the QUERY batch's head index b * H + h and the key index local to the group's range."""
    _check(kind, dev, Geo(**case), torch.bfloat16, fwd_only=fwd_only)


def test_key_stationary_backward_accumulates_on_a_known_buffer(dev):
    """attn_x_bwd_kernel<., ., ACC = true>: accumulate_kv adds dK | dV to what the buffers hold"""
    _parity(dev, Geo(2, 2, 42, 330, bmod=2), torch.bfloat16, acc=True)


@pytest.fixture
def device_rng(dev):
    from valor_amd import ops
    ops.DropoutState.disable_device_base()
    yield ops.DropoutState
    ops.DropoutState.disable_device_base()
    ops.DropoutState.reset(1234)


@KINDS
@pytest.mark.parametrize("dtype,case", [(torch.float32, dict(B=2, H=3, Sq=70, Skv=130)), (torch.bfloat16, dict(B=2, H=2, Sq=129, Skv=129))],
                         ids=["streaming-fp32", "resident-bf16"])
def test_device_resident_base(dev, device_rng, dtype, case, kind):
    """rng_base: the kernels add a 64-bit device counter to the by-value offset when they run (common.h rng_offset); the restatement
    receives the sum. Base 3 * 2^40 + 12345: the high word of the offset enters the head key."""
    base = device_rng.enable_device_base(dev)
    base.fill_(DEVICE_BASE)
    try:
        _check(kind, dev, Geo(**case), dtype, base=DEVICE_BASE)
    finally:
        device_rng.disable_device_base()


# ---------------------------------------------------------------------------------------------- fused two-pass cross-attention
def _fused_geos(case):
    bmod, H, Skv, passes = case
    return [Geo(G * bmod, H, T, Skv, ranges=ranges, bmod=bmod) for G, T, ranges in passes]


def _fused_run(geos, qs, k, v, douts, p, windows):
    from valor_amd import kernels as K
    H, bmod = geos[0].H, geos[0].bmod
    segs = []
    for geo, q, (seed, off) in zip(geos, qs, windows):
        segs.append(dict(q=q, o=torch.full_like(q, float("nan")), lse=torch.full((geo.B, H, geo.Sq), float("nan"), device=q.device),
                         kv_range=geo.kvr_dev, seed=seed, offset=off))
    assert K.cross_attn_fwd_fused(segs, k, v, H, bmod, scale=SCALE, p_drop=p)
    dkv = torch.full((bmod, geos[0].Skv, 2 * geos[0].E), float("nan"), dtype=k.dtype, device=k.device)
    for sg, do in zip(segs, douts):
        sg["dout"], sg["dq"] = do, torch.full_like(sg["q"], float("nan"))
    assert K.cross_attn_bwd_fused(segs, k, v, dkv[:, :, :geos[0].E], dkv[:, :, geos[0].E:], H, bmod, scale=SCALE, p_drop=p)
    torch.cuda.synchronize()
    return [sg["o"] for sg in segs], [sg["dq"] for sg in segs], dkv[:, :, :geos[0].E], dkv[:, :, geos[0].E:]


def _fused_reference(geos, qs, k, v, douts, keeps, p):
    kd, vd = k.double().detach().requires_grad_(True), v.double().detach().requires_grad_(True)
    qds, os_, loss = [], [], 0
    for geo, q, do, keep in zip(geos, qs, douts, keeps):
        qd = q.double().detach().requires_grad_(True)
        o = R.ref_attn_dropout(qd, kd, vd, geo.H, None, geo.kvr, geo.bmod, SCALE, keep, p)
        loss = loss + (o * do.double()).sum()
        qds.append(qd)
        os_.append(o.detach())
    loss.backward()
    return os_, [qd.grad for qd in qds], kd.grad, vd.grad


@KINDS
@pytest.mark.parametrize("ci", [1, 3])
def test_fused_two_pass_cross_attention(dev, ci, kind):
    """attn_xu_fwd_kernel / attn_xu_bwd_kernel (attention_xu.hip) through K.cross_attn_fwd_fused / K.cross_attn_bwd_fused: up to two
    decoder passes over one K | V in one launch, every pass with its own (seed, offset) window, <= ten 16-row query sub-tiles.
    CASES[1] and CASES[3] of test_cross_attn_fused_gpu.py: ranges that start and end inside a 64-key tile, two grouped passes."""
    p = 0.1
    geos = [g.on(dev) for g in _fused_geos(XCASES[ci])]
    bmod, H, Skv, E = geos[0].bmod, geos[0].H, geos[0].Skv, geos[0].E
    windows = [(11 + i, 1000 * (i + 1)) for i in range(len(geos))]
    keeps = [_keep(dev, geo, p, seed, off) for geo, (seed, off) in zip(geos, windows)]
    min_len = min(g.min_len for g in geos)

    def store(kd, vd):
        kv = torch.cat((kd, vd), dim=-1).bfloat16()
        return kv[:, :, :E], kv[:, :, E:]

    if kind == "parity":
        g = torch.Generator().manual_seed(Skv + 7 * bmod)
        k, v = store((torch.randn((bmod, Skv, E), generator=g) * 0.8).to(dev), (torch.randn((bmod, Skv, E), generator=g) * 0.8).to(dev))
        qs = [(torch.randn((geo.B, geo.Sq, E), generator=g) * 0.8).bfloat16().to(dev) for geo in geos]
        douts = [torch.randn((geo.B, geo.Sq, E), generator=g).bfloat16().to(dev) for geo in geos]
        o, dq, dk, dv = _fused_run(geos, qs, k, v, douts, p, windows)
        ro, rdq, rdk, rdv = _fused_reference(geos, qs, k, v, douts, keeps, p)
        errs = {"dk": _rel(dk, rdk), "dv": _rel(dv, rdv)}
        for i in range(len(geos)):
            errs[f"o{i}"], errs[f"dq{i}"] = _rel(o[i], ro[i]), _rel(dq[i], rdq[i])
        print("PARITY fused", XCASES[ci][:3], {n: f"{e:.2e}" for n, e in errs.items()}, "tol 0.01/0.02")
        for n, e in errs.items():
            assert e < (1e-2 if n.startswith("o") else 2e-2), (n, e)
        return
    step = R.keep_scale(p) / min_len
    tol = {"o": 0.25 * step, "dv": 0.25 * step, "dq": 0.25 * step * SCALE, "dk": 0.25 * step * SCALE}
    worst = {}
    probes = [list(_probe_inputs(geo, dev)) for geo in geos]      # the passes share the key chunks; every pass has one query chunk
    assert all(len(pr) == len(probes[0]) for pr in probes)
    for runs in zip(*probes):
        name, outs = runs[0][0], runs[0][1]
        k, v = store(runs[0][3], runs[0][4])
        qs, douts = [r[2].bfloat16() for r in runs], [r[5].bfloat16() for r in runs]
        o, dq, dk, dv = _fused_run(geos, qs, k, v, douts, p, windows)
        ro, rdq, rdk, rdv = _fused_reference(geos, qs, k, v, douts, keeps, p)
        pairs = {"o": list(zip(o, ro)), "dq": list(zip(dq, rdq)), "dk": [(dk, rdk)], "dv": [(dv, rdv)]}
        for n in outs:
            for a, b in pairs[n]:
                err = (a.double() - b).abs().max().item()
                worst[n] = max(worst.get(n, 0.0), err / tol[n])
                assert err < tol[n], (name, n, err, tol[n])
    print("PROBES fused", XCASES[ci][:3], "worst error / accepted:", {n: f"{e:.3f}" for n, e in worst.items()})
