"""Every attention kernel family on HARD softmax rows (tests/attn_hard_inputs.py: peaked, tie, ramp-up / ramp-down, +-80 nat shifted and
intruder rows beside benign ones), with dense finite masks, masks whose closed regions matter, scale != 1/8 -- o, lse, dq, dk, dv against
explicit fp64 attention. tests/test_attn_hard_inputs_cpu.py holds the inputs to their classes.

Errors: o and dq relative L2 PER ROW CLASS (a wrong rescale on the ramp rows is not diluted by the benign ones), dk / dv relative L2 over
the tensor, lse maximum absolute error per class. Rows whose reference P is one-hot have dQ ~ 0: their dQ error is taken against
max(class norm, tensor rms * sqrt(class numel)). Without a mask these are the peaked rows (and intruder rows whose intruding key only a
`blocked` mask would close); under a mask tie and intruder rows too (_onehot).

Bounds. bf16 kernels: the project's 1e-2 (o) and 2e-2 (gradients; 1.5e-2 for window attention) -- P is rounded to bf16 ahead of P.V at
any score range. fp32 kernels, and lse in both dtypes: max(project tolerance, 4 x the error of the SAME formula evaluated in plain fp32
torch on the same inputs and the same class) with the project tolerances 3e-6 (o), 1e-5 (gradients), 1e-5 absolute (lse), 2e-5 (fp32
window attention): an fp32 score of 80 nats carries 4e-6 of absolute error in any implementation; the factor 4 covers another summation
order of the 64-term dot products and the hardware exponential. The fp32 yardstick of o and lse is attn_hard_inputs.ref_fp32; of the
gradients attn_hard_inputs.grads_lse, the backward from the STORED fp32 o and lse (P = exp(s - lse)) that the C interface gives every
backward kernel: a row whose every key carries -10000 has an lse with an ulp of 1e-3, which reaches P whatever the kernel does (autograd
through a softmax that never forms lse does not see it; in fp64 the two agree to 1e-10, tests/test_attn_hard_inputs_cpu.py).

Measured on an MI355X (worst case over the cases of a family, error / bound; `decode` rows: the decode kernel's o and lse, and the
backward kernels on that lse; closed rows of the `blocked` masks set the 1e-4 .. 1e-3 figures of the masked families):
  family / dtype             tensor           benign           peaked              tie           rampup         rampdown          shifted         intruder
  decode bf16                o       2.4e-03/1.0e-02  1.7e-03/1.0e-02  1.9e-03/1.0e-02  2.3e-03/1.0e-02  2.3e-03/1.0e-02  2.2e-03/1.0e-02  1.8e-03/1.0e-02
  decode bf16                dq      7.2e-03/2.0e-02  6.9e-03/2.0e-02  8.8e-03/2.0e-02  1.5e-02/2.0e-02  5.1e-03/2.0e-02  4.2e-03/2.0e-02  1.3e-02/2.0e-02
  decode bf16                lse     3.7e-04/1.5e-03  1.9e-06/1.0e-05  2.9e-06/1.2e-05  4.4e-06/1.8e-05  4.4e-04/1.8e-03  7.0e-06/1.0e-05  4.6e-07/1.0e-05
  decode bf16                dk 4.7e-03/2.0e-02   dv 2.2e-03/2.0e-02
  decode fp32                o       2.1e-04/8.5e-04  2.7e-07/3.0e-06  1.3e-07/3.0e-06  9.9e-07/3.1e-06  1.7e-06/5.5e-06  7.5e-06/2.6e-05  1.7e-07/3.0e-06
  decode fp32                dq      1.4e-04/5.7e-04  6.0e-07/1.0e-05  2.1e-04/8.3e-04  1.7e-05/2.1e-05  4.6e-04/1.9e-03  2.2e-05/2.6e-05  1.1e-06/1.0e-05
  decode fp32                lse     3.7e-04/1.5e-03  1.9e-06/1.0e-05  2.9e-06/1.2e-05  4.4e-06/1.8e-05  4.4e-04/1.8e-03  7.0e-06/1.0e-05  5.0e-07/1.0e-05
  decode fp32                dk 2.0e-05/2.1e-05   dv 4.6e-06/1.3e-05
  fused bf16                 o       2.3e-03/1.0e-02  1.2e-12/1.0e-02  1.8e-03/1.0e-02  2.1e-03/1.0e-02  2.1e-03/1.0e-02  2.3e-03/1.0e-02  1.6e-03/1.0e-02
  fused bf16                 dq      5.7e-03/2.0e-02  2.9e-07/2.0e-02  5.6e-03/2.0e-02  8.9e-03/2.0e-02  3.5e-03/2.0e-02  4.8e-03/2.0e-02  7.9e-03/2.0e-02
  fused bf16                 lse     1.1e-06/1.0e-05  5.0e-12/1.0e-05  1.4e-06/1.0e-05  7.5e-06/3.1e-05  4.5e-06/2.9e-05  6.9e-06/1.9e-05  2.3e-06/1.0e-05
  fused bf16                 dk 2.8e-03/2.0e-02   dv 2.4e-03/2.0e-02
  key-stationary bf16        o       2.2e-03/1.0e-02  4.9e-13/1.0e-02  1.8e-03/1.0e-02  2.1e-03/1.0e-02  2.2e-03/1.0e-02  2.2e-03/1.0e-02  1.7e-03/1.0e-02
  key-stationary bf16        dq      4.5e-03/2.0e-02  2.6e-07/2.0e-02  5.2e-03/2.0e-02  1.2e-02/2.0e-02  4.3e-03/2.0e-02  4.9e-03/2.0e-02  7.3e-03/2.0e-02
  key-stationary bf16        lse     8.6e-07/1.0e-05  3.8e-06/1.0e-05  1.4e-06/1.0e-05  8.5e-06/2.7e-05  4.2e-06/2.1e-05  7.1e-06/2.0e-05  1.9e-06/1.0e-05
  key-stationary bf16        dk 2.6e-03/2.0e-02   dv 1.9e-03/2.0e-02
  resident bf16              o       2.4e-03/1.0e-02  8.6e-04/1.0e-02  1.9e-03/1.0e-02  2.1e-03/1.0e-02  2.1e-03/1.0e-02  2.3e-03/1.0e-02  1.4e-03/1.0e-02
  resident bf16              dq      8.0e-03/2.0e-02  3.2e-03/2.0e-02  9.2e-03/2.0e-02  1.0e-02/2.0e-02  4.4e-03/2.0e-02  7.4e-03/2.0e-02  6.6e-03/2.0e-02
  resident bf16              lse     7.5e-04/1.3e-03  7.4e-06/1.0e-05  7.1e-06/1.1e-05  6.8e-04/2.0e-03  6.5e-04/1.7e-03  6.5e-04/1.3e-03  2.3e-06/1.0e-05
  resident bf16              dk 4.9e-03/2.0e-02   dv 2.0e-03/2.0e-02
  resident-dropout bf16      o       2.3e-03/1.0e-02  2.3e-03/1.0e-02  2.3e-03/1.0e-02  2.3e-03/1.0e-02  2.3e-03/1.0e-02  2.3e-03/1.0e-02                -
  resident-dropout bf16      dq      6.9e-03/2.0e-02  1.2e-02/2.0e-02  1.0e-02/2.0e-02  9.2e-03/2.0e-02  5.9e-03/2.0e-02  7.4e-03/2.0e-02                -
  resident-dropout bf16      lse     1.4e-06/1.0e-05  8.6e-06/1.5e-05  7.6e-06/1.2e-05  3.6e-06/2.3e-05  9.3e-07/1.0e-05  2.0e-05/7.9e-05                -
  resident-dropout bf16      dk 4.8e-03/2.0e-02   dv 2.5e-03/2.0e-02
  resident-persistent bf16   o       2.2e-03/1.0e-02  6.4e-04/1.0e-02  1.8e-03/1.0e-02  2.1e-03/1.0e-02  2.1e-03/1.0e-02  2.2e-03/1.0e-02  1.4e-03/1.0e-02
  resident-persistent bf16   dq      4.6e-03/2.0e-02  3.6e-03/2.0e-02  6.7e-03/2.0e-02  7.0e-03/2.0e-02  4.5e-03/2.0e-02  4.6e-03/2.0e-02  6.2e-03/2.0e-02
  resident-persistent bf16   lse     8.1e-04/2.1e-03  8.6e-06/1.5e-05  6.6e-06/1.3e-05  8.8e-04/2.7e-03  9.1e-04/2.8e-03  7.8e-04/2.1e-03  2.8e-06/1.0e-05
  resident-persistent bf16   dk 3.1e-03/2.0e-02   dv 2.0e-03/2.0e-02
  scale=0.3 bf16             o       2.0e-03/1.0e-02                -                -                -                -                -                -
  scale=0.3 bf16             dq      2.7e-03/2.0e-02                -                -                -                -                -                -
  scale=0.3 bf16             lse     8.5e-07/1.0e-05                -                -                -                -                -                -
  scale=0.3 bf16             dk 2.5e-03/2.0e-02   dv 2.4e-03/2.0e-02
  scale=0.3 fp32             o       3.0e-07/3.0e-06                -                -                -                -                -                -
  scale=0.3 fp32             dq      4.0e-07/1.0e-05                -                -                -                -                -                -
  scale=0.3 fp32             lse     7.0e-07/1.0e-05                -                -                -                -                -                -
  scale=0.3 fp32             dk 3.6e-07/1.0e-05   dv 3.2e-07/1.0e-05
  streaming bf16             o       2.2e-03/1.0e-02  8.6e-04/1.0e-02  1.9e-03/1.0e-02  2.0e-03/1.0e-02  2.1e-03/1.0e-02  2.2e-03/1.0e-02  1.3e-03/1.0e-02
  streaming bf16             dq      8.0e-03/2.0e-02  2.2e-03/2.0e-02  1.1e-02/2.0e-02  6.5e-03/2.0e-02  5.2e-03/2.0e-02  7.4e-03/2.0e-02  6.6e-03/2.0e-02
  streaming bf16             lse     4.6e-04/1.8e-03  2.9e-06/1.1e-05  2.9e-06/1.2e-05  3.5e-06/1.3e-05  4.6e-04/1.8e-03  4.4e-04/1.8e-03  1.7e-06/1.0e-05
  streaming bf16             dk 4.9e-03/2.0e-02   dv 2.0e-03/2.0e-02
  streaming fp32             o       6.5e-05/2.6e-04  5.3e-08/3.0e-06  4.7e-07/3.0e-06  4.8e-06/1.2e-05  1.2e-04/4.7e-04  6.8e-06/2.5e-05  2.1e-07/3.0e-06
  streaming fp32             dq      1.3e-04/5.3e-04  5.0e-07/1.0e-05  1.7e-04/6.7e-04  4.9e-06/1.5e-05  6.7e-05/2.7e-04  1.2e-05/3.5e-05  7.9e-07/1.0e-05
  streaming fp32             lse     4.6e-04/1.8e-03  2.9e-06/1.1e-05  2.9e-06/1.2e-05  5.1e-06/1.3e-05  4.6e-04/1.8e-03  3.0e-05/7.1e-05  1.7e-06/1.0e-05
  streaming fp32             dk 1.2e-05/3.6e-05   dv 7.3e-05/2.9e-04
  window bf16                o       2.1e-03/1.0e-02  8.2e-04/1.0e-02  1.5e-03/1.0e-02                -                -  2.2e-03/1.0e-02                -
  window bf16                dq      2.9e-03/1.5e-02  3.8e-03/1.5e-02  1.4e-02/1.5e-02                -                -  3.0e-03/1.5e-02                -
  window bf16                lse     2.4e-06/1.0e-05  9.2e-06/1.9e-04  1.6e-05/2.0e-04                -                -  1.4e-05/7.0e-05                -
  window bf16                dk 2.7e-03/1.5e-02   dv 2.0e-03/1.5e-02   dtable 2.5e-03/1.5e-02
  window fp32                o       3.8e-07/2.0e-05  3.6e-07/2.0e-05  1.6e-06/2.0e-05                -                -  1.6e-05/4.8e-05                -
  window fp32                dq      1.0e-06/2.0e-05  1.2e-06/3.2e-05  2.1e-06/2.0e-05                -                -  1.2e-05/3.4e-05                -
  window fp32                lse     2.4e-06/1.0e-05  9.2e-06/1.9e-04  1.6e-05/2.0e-04                -                -  3.7e-05/1.2e-04                -
  window fp32                dk 1.3e-05/3.7e-05   dv 5.0e-06/2.0e-05   dtable 9.6e-06/2.4e-05
"""
import contextlib
import types

import numpy as np
import pytest
import torch

import attn_hard_inputs as A
import dropout_ref as R
from test_cross_attn_fused_gpu import CASES as XCASES

pytestmark = pytest.mark.gpu
RANGES2 = [(0, 200), (37, 101)]
RANGES3 = [(0, 330), (21, 190), (150, 167)]         # edges inside 64-key tiles
RANGES4 = [(0, 330), (21, 190), (150, 167), (70, 64)]
F32, BF16 = torch.float32, torch.bfloat16
_REFS = {}


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


def _benign(B, H, Sq, Skv, bmod=0):
    """the input regime of the other attention tests (for the scale cases): randn * 0.8, every row of class benign"""
    g = torch.Generator().manual_seed(B * 1000 + Sq + Skv)
    E, Bkv = H * 64, (bmod if bmod > 0 else B)
    mk = lambda *s: (torch.randn(s, generator=g) * 0.8).bfloat16().float()
    return types.SimpleNamespace(q=mk(B, Sq, E), k=mk(Bkv, Skv, E), v=mk(Bkv, Skv, E), dout=mk(B, Sq, E), kv_range=None, bmod=bmod,
                                   H=H, cls=torch.zeros((B, Sq), dtype=torch.int64), intr_local=torch.full((B,), -1), intruder=None)


def _prepared(B, H, Sq, Skv, ranges=None, bmod=0, mask="none", scale=0.125, p=0.0, sel=None, first=0, benign=False):
    """inputs, mask, keep mask and both references of one case, computed once on the host and shared by every kernel variant that runs it.
    sel: the batches the references cover (the many-item shapes)."""
    key = (B, H, Sq, Skv, tuple(ranges) if ranges else None, bmod, mask, scale, p, sel, first, benign)
    if key not in _REFS:
        h = _benign(B, H, Sq, Skv, bmod) if benign else A.make(B, H, Sq, Skv, ranges, bmod, first=first)
        m = A.masks(B, Sq, Skv, mask, hard=h)
        cls = h.cls.clone()
        if h.intruder == "mask" and mask != "blocked":        # the intruding key is open: these rows are one-hot on it
            cls[cls == A.INTRUDER] = A.PEAKED
        keep = None
        if p > 0:
            heads = np.array([b * H + hh for b in (sel if sel is not None else range(B)) for hh in range(H)])
            keep = torch.from_numpy(R.attn_keep_heads(5, 9, heads, Sq, Skv, p).reshape(-1, H, Sq, Skv))
        ix = torch.tensor(sel) if sel is not None else None
        pick = (lambda t: t[ix]) if sel is not None else (lambda t: t)
        kw = dict(mask=(m if m is None or m.shape[0] == 1 else pick(m)), kv_range=(pick(h.kv_range) if h.kv_range is not None else None),
                  bmod=bmod, scale=scale, keep=keep, p=float(np.float32(p)))
        assert sel is None or bmod == 0
        args = (pick(h.q), pick(h.k) if bmod == 0 else h.k, pick(h.v) if bmod == 0 else h.v, pick(h.dout), H)
        _REFS[key] = (h, m, pick(cls), A.grads(*args, **kw), A.grads_lse(*args, dtype=F32, **kw))
    return _REFS[key]


def _store(h, dtype, dev):
    """q, k, v as strided views of fused buffers (row stride 3E / 2E), as the model keeps them"""
    E = h.q.shape[-1]
    if h.q.shape == h.k.shape and h.kv_range is None and h.bmod == 0:
        buf = torch.cat((h.q, h.k, h.v), dim=-1).to(dtype).to(dev)
        return buf[:, :, :E], buf[:, :, E:2 * E], buf[:, :, 2 * E:]
    qb = torch.cat((h.q, torch.zeros_like(h.q), torch.zeros_like(h.q)), dim=-1).to(dtype).to(dev)
    kvb = torch.cat((h.k, h.v), dim=-1).to(dtype).to(dev)
    return qb[:, :, :E], kvb[:, :, :E], kvb[:, :, E:]


def _launch(dev, dtype, h, m, scale, p=0.0):
    from valor_amd import kernels as K
    q, k, v = _store(h, dtype, dev)
    dout = h.dout.to(dtype).to(dev)
    kw = dict(mask=m.to(dev) if m is not None else None, kv_range=h.kv_range.to(dev) if h.kv_range is not None else None, kv_bmod=h.bmod,
              scale=scale, p_drop=p, seed=5, offset=9)
    o, lse = K.attn_fwd(q, k, v, h.H, **kw)
    dq, dk, dv = K.attn_bwd(q, k, v, o, lse, dout, h.H, **kw)
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _rel(a, b, floor=0.0):
    return ((a.double() - b.double()).norm() / max(b.double().norm().item(), floor, 1e-30)).item()


def _errors(got, ref, cls, names, onehot=(A.PEAKED,)):
    """{(tensor, class name | 'all'): error} of `got` against `ref`; cls [B, Sq]; o / dq [B, Sq, E], lse [B, H, Sq]"""
    out = {}
    for c in sorted(set(cls.reshape(-1).tolist())):
        sel, cn = cls == c, names[c]
        out[("o", cn)] = _rel(got["o"][sel], ref["o"][sel])
        if "dq" in got:
            floor = ref["dq"].double().pow(2).mean().sqrt().item() * ref["dq"][sel].numel() ** 0.5 if c in onehot else 0.0
            out[("dq", cn)] = _rel(got["dq"][sel], ref["dq"][sel], floor)
        if "lse" in got:
            out[("lse", cn)] = (got["lse"].double() - ref["lse"].double()).transpose(1, 2)[sel].abs().max().item()
    for n in ("dk", "dv"):
        if n in got:
            out[(n, "all")] = _rel(got[n], ref[n])
    return out


def _judge(tag, family, dtype, got, r64, r32, cls, names=A.CLASSES, onehot=(A.PEAKED,), tol=None):
    got = {n: t.detach().float().cpu() for n, t in got.items() if t is not None}
    for n, t in got.items():
        assert torch.isfinite(t).all(), (tag, n, "not finite")
    err, e32 = _errors(got, r64, cls, names, onehot), _errors(r32, r64, cls, names, onehot)
    tol_o, tol_g, tol_lse = tol or ((3e-6, 1e-5, 1e-5) if dtype == F32 else (1e-2, 2e-2, 1e-5))
    fails, line = [], []
    for (n, cn), e in err.items():
        base = tol_lse if n == "lse" else tol_o if n == "o" else tol_g
        bound = max(base, 4 * e32[(n, cn)]) if (dtype == F32 or n == "lse") else base
        line.append(f"{n}[{cn}] {e:.2e}/{bound:.2e}")
        if not e < bound:
            fails.append((n, cn, e, bound))
    print("HARD", tag, str(dtype)[6:], " ".join(line))
    assert not fails, (tag, fails)


def _onehot(mask):
    """the classes whose reference dQ can be ~0. Without a mask: peaked. Under a mask tie and intruder rows as well: N(0, 3) mask values
    split a tie by several nats, a closed tie partner or tile leaves ONE dominant key -- P is one-hot to 1e-3 and better on most of them."""
    return (A.PEAKED,) if mask == "none" else (A.PEAKED, A.TIE, A.INTRUDER)


def _attn_case(dev, family, dtype, geo, mask="none", scale=0.125, p=0.0, sel=None, first=0, benign=False):
    h, m, cls, r64, r32 = _prepared(*geo, mask=mask, scale=scale, p=p, sel=sel, first=first, benign=benign)
    got = _launch(dev, dtype, h, m, scale, p)
    if sel is not None:
        ix = torch.tensor(sel, device=dev)
        got = {n: t[ix] for n, t in got.items()}
    tag = f"{family} {geo[:4]}{' ranged' if len(geo) > 4 and geo[4] else ''} mask={mask} scale={scale:g} p={p}"
    _judge(tag, family, dtype, got, r64, r32, cls, onehot=_onehot(mask))


# ---------------------------------------------------------------------------------------------- streaming kernels
STREAM = [((2, 2, 70, 130), m) for m in ("none", "dense", "dense1", "blocked")] + [((2, 2, 33, 33), m) for m in ("none", "dense", "dense1", "blocked")] \
    + [((4, 2, 48, 200, RANGES2, 2), "none")]
_sid = lambda c: "x".join(str(v) for v in c[0][:4]) + "-" + c[1]      # noqa: E731


@pytest.mark.parametrize("case", STREAM, ids=_sid)
def test_streaming_fp32(dev, case):
    """attn_fwd_kernel<float> / attn_bwd_dq_kernel<float> / attn_bwd_dkv_kernel<float>: the online softmax over 64-key tiles (rescale by
    exp(m_old - m_new), the -1e30 start of the running maximum), the mask gather of both backward kernels, lse re-used by both"""
    _attn_case(dev, "streaming", F32, case[0], case[1])


@pytest.mark.parametrize("case", STREAM, ids=_sid)
def test_streaming_bf16(dev, case):
    with _family(variant=0):
        _attn_case(dev, "streaming", BF16, case[0], case[1])


# ---------------------------------------------------------------------------------------------- LDS-resident kernels
@pytest.mark.parametrize("mask", ["none", "dense", "blocked"])
@pytest.mark.parametrize("pipe", [0, 1, 2])
@pytest.mark.parametrize("S", [33, 65, 160, 161, 256])
def test_resident(dev, S, pipe, mask):
    """attn_res_fwd_kernel and, by S and valor_attn_set_res_pipeline: S = 33 attn_res_bwd1_kernel (one wave); S = 65, 160 attn_res_bwd16_kernel
    in modes 1, 2 and attn_res_bwd_kernel in mode 0; S = 161, 256 attn_res_bwd_kernel in modes 0, 1 (4 items: nothing to pipeline) and
    attn_res_bwd16_kernel in mode 2 -- every one with and without its MASK instantiation"""
    with _family(pipe=pipe):
        _attn_case(dev, "resident", BF16, (2, 2, S, S), mask)


def _many(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    B = -(-2 * cus // 12) + 1
    assert B * 12 >= 2 * cus
    return (B, 12, 161, 161), (0, B // 2, B - 1)


@pytest.mark.parametrize("mask", ["none", "dense", "blocked"])
@pytest.mark.parametrize("pipe", [1, 3])
def test_resident_many_items(dev, pipe, mask):
    """B * H >= 2 x CUs items of 161 rows: attn_res_bwd_pipe2_kernel (mode 1, no mask) and attn_res_bwd_pipe_kernel (mode 3; mode 1 with a
    mask: the second version has no masked instantiation) -- with and without MASK. fp64 on the first, a middle and the last batch."""
    geo, sel = _many(dev)
    with _family(pipe=pipe):
        _attn_case(dev, "resident-persistent", BF16, geo, mask, sel=sel)


@pytest.mark.parametrize("S,pipe", [(33, 1), (100, 1), (197, 0), (0, 1)], ids=["bwd1", "bwd16", "bwd8", "persistent"])
def test_resident_masked_backward_with_dropout(dev, S, pipe):
    """the <DROP, MASK> instantiation of every resident backward: a dense mask and p = 0.1, the keep mask restated by tests/dropout_ref.py"""
    geo, sel = ((2, 2, S, S), None) if S else _many(dev)
    with _family(pipe=pipe):
        _attn_case(dev, "resident-dropout", BF16, geo, "dense", p=0.1, sel=sel)


# ---------------------------------------------------------------------------------------------- key-stationary cross-attention
@pytest.mark.parametrize("geo", [(2, 2, 32, 458), (6, 2, 16, 330, RANGES3, 2), (6, 2, 32, 330, RANGES3, 2), (8, 2, 32, 330, RANGES4, 2)],
                         ids=lambda g: "x".join(str(v) for v in g[:4]))
def test_key_stationary(dev, geo):
    """attn_x_fwd_kernel (2, 3 -> 4, 6 and 8 query sub-tiles: the four-wave state merge, keys outside the group's range at -inf) and
    attn_x_bwd_kernel (the first two; the last two take the streaming backward with the key-stationary forward's lse)"""
    h = _prepared(*geo)[0]
    if len(geo) > 4:
        assert (h.cls == A.INTRUDER).any()
    _attn_case(dev, "key-stationary", BF16, geo)


# ---------------------------------------------------------------------------------------------- fused two-pass cross-attention
def _fused_case(dev, ci, scale=0.125, benign=False):
    from valor_amd import kernels as K
    bmod, H, Skv, passes = XCASES[ci]
    key = ("fused", ci, scale, benign)
    if key not in _REFS:
        k, v, ps = A.make_passes(H, Skv, bmod, passes)
        if benign:
            g = torch.Generator().manual_seed(ci)
            mk = lambda t: (torch.randn(t.shape, generator=g) * 0.8).bfloat16().float()
            k, v = mk(k), mk(v)
            for h in ps:
                h.q, h.k, h.v, h.cls = mk(h.q), k, v, torch.zeros_like(h.cls)
        kd, vd = k.double().requires_grad_(True), v.double().requires_grad_(True)
        qds, outs, loss = [], [], 0
        for h in ps:
            qd = h.q.double().requires_grad_(True)
            o, lse = A.ref(qd, kd, vd, H, kv_range=h.kv_range, bmod=bmod, scale=scale)
            loss = loss + (o * h.dout.double()).sum()
            qds.append(qd)
            outs.append((o.detach(), lse.detach()))
        loss.backward()
        r64 = [dict(o=o, lse=lse, dq=qd.grad, dk=kd.grad, dv=vd.grad) for (o, lse), qd in zip(outs, qds)]
        r32 = [A.grads_lse(h.q, k, v, h.dout, H, kv_range=h.kv_range, bmod=bmod, scale=scale) for h in ps]
        for r in r32:                  # dK | dV of the launch: the sum over its passes
            r["dk"], r["dv"] = sum(x["dk"] for x in r32), sum(x["dv"] for x in r32)
        refs = [r64, r32]
        _REFS[key] = (k, v, ps, refs[0], refs[1])
    k, v, ps, r64, r32 = _REFS[key]
    E = H * 64
    kv = torch.cat((k, v), -1).bfloat16().to(dev)
    kd, vd = kv[:, :, :E], kv[:, :, E:]
    segs = []
    for h in ps:
        q = h.q.bfloat16().to(dev)
        segs.append(dict(q=q, o=torch.full_like(q, float("nan")), lse=torch.full((q.shape[0], H, q.shape[1]), float("nan"), device=dev),
                         kv_range=h.kv_range.to(dev) if h.kv_range is not None else None, seed=0, offset=0))
    assert K.cross_attn_fwd_fused(segs, kd, vd, H, bmod, scale=scale)
    dkv = torch.full_like(kv, float("nan"))
    for sg, h in zip(segs, ps):
        sg["dout"], sg["dq"] = h.dout.bfloat16().to(dev), torch.full_like(sg["q"], float("nan"))
    assert K.cross_attn_bwd_fused(segs, kd, vd, dkv[:, :, :E], dkv[:, :, E:], H, bmod, scale=scale)
    torch.cuda.synchronize()
    for i, (sg, h) in enumerate(zip(segs, ps)):
        got = dict(o=sg["o"], lse=sg["lse"], dq=sg["dq"])
        if i == 0:
            got.update(dk=dkv[:, :, :E], dv=dkv[:, :, E:])
        _judge(f"fused case {ci} pass {i} scale={scale:g}", "fused", BF16, got, r64[i], r32[i], h.cls)


@pytest.mark.parametrize("ci", [1, 2])
def test_fused_two_pass(dev, ci):
    """attn_xu_fwd_kernel / attn_xu_bwd_kernel on the second and third geometry of test_cross_attn_fused_gpu.CASES (Skv = 330 with ranges
    whose edges are each other's intruders, two passes; Skv = 64 with a query tail), hard rows per pass over one planned K | V"""
    _fused_case(dev, ci)


# ---------------------------------------------------------------------------------------------- decode step
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mask", ["dense", "blocked"])
@pytest.mark.parametrize("geo,first", [((5, 2, 2, 41), 0), ((3, 2, 4, 65), 0), ((2, 2, 1, 256), 0), ((2, 2, 1, 256), 3)],
                         ids=lambda g: "x".join(str(v) for v in g) if isinstance(g, tuple) else f"first{g}")
def test_decode_step(dev, geo, first, mask, dtype):
    """attn_dec_fwd_kernel through valor_attn_fwd (variant bit 4) and through valor_attn_decode_fwd: o and lse against fp64, and the
    backward kernels on the decode kernel's lse. (2, 2, 1, 256) holds two rows: it runs with the class cycle started at 0 and at 3.)"""
    from valor_amd import kernels as K, lib
    assert lib.load().valor_attn_set_variant(-1) & 4
    _attn_case(dev, "decode", dtype, geo, mask, first=first)
    h, m, cls, r64, r32 = _prepared(*geo, mask=mask, first=first)
    q, k, v = _store(h, dtype, dev)
    o = K.attn_decode(q, k, v, h.H, mask=m.to(dev))
    _judge(f"attn_decode {geo} mask={mask}", "decode", dtype, dict(o=o), r64, r32, cls, onehot=_onehot(mask))


# ---------------------------------------------------------------------------------------------- scale
@pytest.mark.parametrize("family", ["streaming-fp32", "streaming-bf16", "resident-33", "resident-100", "resident-197", "key-stationary", "fused",
                                    "decode"])
def test_scale_is_applied_everywhere(dev, family):
    """scale = 0.3 on the benign inputs of the other tests: a kernel that used p.scale in one place and 1/8 in another fails"""
    if family == "fused":
        return _fused_case(dev, 1, scale=0.3, benign=True)
    geo, dtype, variant = {"streaming-fp32": ((2, 2, 70, 130), F32, None), "streaming-bf16": ((2, 2, 70, 130), BF16, 0),
                           "resident-33": ((2, 2, 33, 33), BF16, None), "resident-100": ((2, 2, 100, 100), BF16, None),
                           "resident-197": ((2, 2, 197, 197), BF16, None), "key-stationary": ((2, 2, 32, 458), BF16, None),
                           "decode": ((3, 2, 4, 65), F32, None)}[family]
    with _family(variant=variant):
        _attn_case(dev, "scale " + family, dtype, geo, scale=0.3, benign=True)


# ---------------------------------------------------------------------------------------------- window attention
_MODELS = {}


@pytest.mark.parametrize("dtype,variant", [(BF16, 7), (BF16, 127), (BF16, 0), (F32, 7)], ids=["bf16-v7", "bf16-v127", "bf16-v0", "fp32"])
@pytest.mark.parametrize("size,shifted", [((2, 7, 7), False), ((4, 7, 7), False), ((4, 14, 14), True), ((8, 7, 7), False)],
                         ids=["2x7x7", "4x7x7", "4x14x14s", "8x7x7"])
def test_window_attention(dev, size, shifted, dtype, variant):
    """valor_win_attn_fwd / bwd (head_dim 32) on benign / peaked / tie / shifted rows placed by window slot, with a bias table whose +-20
    entries decide rows' maxima: o, lse, dqkv and dtable against fp64 (the reference of tests/test_swin_gpu.py, and its restatement in
    attn_hard_inputs.ref_window for lse and the fp32 yardstick)"""
    from test_swin_gpu import _model, _ref_window_attention
    from valor_amd import kernels as K, lib, synth
    if dtype not in _MODELS:
        _MODELS[dtype] = _model(dev, dtype)
    model = _MODELS[dtype]
    window, heads, B = model.spec.swin_window, 2, 2
    C = heads * 32
    D, H, W = size
    geo = model._swin_geometry(D, H, W, shifted)
    nW, N = geo["nW"], geo["N"]
    key = ("win", size, shifted)
    if key not in _REFS:
        rowmap = geo["rowmap"].cpu().long()
        label = geo["label"].cpu() if geo["label"] is not None else None
        rel = synth.swin_relative_position_index(window)[:N, :N].long()
        w = A.make_window(B, heads, rowmap, nW, N, model.spec.swin_table)
        wa = (w.qkv, w.table, w.dout, heads, rowmap, label, rel, nW, N)
        refs = [A.grads_window(*wa), A.grads_window(*wa, dtype=F32, via_lse=True)]
        mine = refs[0]
        xr, tr = w.qkv.double().requires_grad_(True), w.table.double().requires_grad_(True)
        theirs = _ref_window_attention(xr.view(B, D, H, W, 3 * C), tr, heads, size, window, shifted)
        theirs.backward(w.dout.double().view(B, D, H, W, C))
        assert _rel(mine["o"], theirs.reshape(B, -1, C)) < 1e-12 and _rel(mine["dqkv"], xr.grad) < 1e-12 and _rel(mine["dtable"], tr.grad) < 1e-12
        # lse [B * nW, heads, N] by window slot -> [B, heads, rows] by row, like an attention lse
        unslot = lambda l: torch.empty((B, heads, nW * N), dtype=l.dtype).index_copy(2, rowmap, l.view(B, nW, heads, N).transpose(1, 2).reshape(B, heads, -1))
        _REFS[key] = (w, rowmap, unslot, refs)
    w, rowmap, unslot, (r64, r32) = _REFS[key]
    old = lib.load().valor_win_attn_set_variant(variant)
    try:
        qkv = w.qkv.to(dtype).to(dev).reshape(-1, 3 * C)
        table = w.table.to(dtype).to(dev)
        o, lse = K.win_attn_fwd(qkv, geo, table, heads, B)
        dqkv, dtable = K.win_attn_bwd(qkv, o, lse, w.dout.to(dtype).to(dev).reshape(-1, C), geo, table, heads, B)
        torch.cuda.synchronize()
    finally:
        lib.load().valor_win_attn_set_variant(old)
    split = lambda t: dict(dq=t[..., :C], dk=t[..., C:2 * C], dv=t[..., 2 * C:])
    got = dict(o=o.float().cpu().view(B, -1, C), lse=unslot(lse.float().cpu()), **split(dqkv.float().cpu().view(B, -1, 3 * C)))
    want = [dict(o=r["o"], lse=unslot(r["lse"]), **split(r["dqkv"])) for r in (r64, r32)]
    tag = f"window {size}{' shifted' if shifted else ''} variant={variant}"
    tol = (2e-5, 2e-5, 1e-5) if dtype == F32 else (1e-2, 1.5e-2, 1e-5)       # the window tests' 2e-5 / 1.5e-2; o in bf16 at the issue's 1e-2
    _judge(tag, "window", dtype, got, want[0], want[1], w.cls, names=A.WIN_CLASSES, onehot=(1, 2), tol=tol)      # the bias turns most ties one-hot
    e, e32 = _rel(dtable.float().cpu(), r64["dtable"]), _rel(r32["dtable"], r64["dtable"])
    bound = max(2e-5, 4 * e32) if dtype == F32 else 1.5e-2
    print("HARD", tag, f"dtable {e:.2e}/{bound:.2e}")
    assert torch.isfinite(dtable.float()).all() and e < bound, ("dtable", e, bound)
