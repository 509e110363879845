"""The hard attention inputs (tests/attn_hard_inputs.py) ARE hard: on the fp64 reference, for every shape of the GPU matrix of
tests/test_attention_hard_gpu.py, each row class has the property it is named after -- so the GPU tests cannot quietly degenerate into
the benign regime of the other attention tests."""
import pytest
import torch

import attn_hard_inputs as A

RANGES2 = [(0, 200), (37, 101)]
RANGES3 = [(0, 330), (21, 190), (150, 167)]
RANGES4 = [(0, 330), (21, 190), (150, 167), (70, 64)]
# B, H, Sq, Skv, ranges, bmod -- the geometries of test_attention_hard_gpu.py (H = 2 stands for the many-item shape's 12 heads)
SHAPES = [
    (2, 2, 70, 130, None, 0), (2, 2, 33, 33, None, 0), (4, 2, 48, 200, RANGES2, 2),                                  # streaming
    (2, 2, 65, 65, None, 0), (2, 2, 100, 100, None, 0), (2, 2, 160, 160, None, 0), (2, 2, 161, 161, None, 0),          # resident
    (2, 2, 197, 197, None, 0), (2, 2, 256, 256, None, 0),
    (2, 2, 32, 458, None, 0), (6, 2, 16, 330, RANGES3, 2), (6, 2, 32, 330, RANGES3, 2), (8, 2, 32, 330, RANGES4, 2),   # key-stationary
    (2, 2, 20, 64, None, 2),                                                                                          # fused, one pass
    (5, 2, 2, 41, None, 0), (3, 2, 4, 65, None, 0), (2, 2, 1, 256, None, 0), (2, 2, 4, 41, None, 0),                   # decode step
]


def _scores(h, H, b, hd=64):
    """fp64 scaled scores [H, Sq, len] of batch b over the keys it may see, and over the whole buffer"""
    kb = b % h.bmod if h.bmod > 0 else b
    Sq = h.q.shape[1]
    qq = h.q[b].double().view(Sq, H, hd).transpose(0, 1)
    kk = h.k[kb].double().view(-1, H, hd).transpose(0, 1)
    full = qq @ kk.transpose(1, 2) * 0.125
    s0, ln = (0, h.k.shape[1]) if h.kv_range is None else (int(h.kv_range[b, 0]), int(h.kv_range[b, 1]))
    return full[:, :, s0:s0 + ln], full


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]) + ("-ranged" if s[4] else ""))
def test_classes_have_their_properties(shape):
    B, H, Sq, Skv, ranges, bmod = shape
    h = A.make(B, H, Sq, Skv, ranges, bmod)
    kw = dict(kv_range=h.kv_range, bmod=bmod)
    o, lse = A.ref(h.q, h.k, h.v, H, **kw)
    present = set(h.cls.reshape(-1).tolist())
    if B * Sq >= 7:
        assert len(present) >= 6, f"classes present: {[A.CLASSES[c] for c in sorted(present)]}"
    for b in range(B):
        s, _ = _scores(h, H, b)
        P = torch.softmax(s, -1)
        ln = s.shape[-1]
        for r in range(Sq):
            c = int(h.cls[b, r])
            top = P[:, r].sort(-1, descending=True).values
            if c == A.PEAKED:
                assert (top[:, 0] >= 1 - 1e-9).all(), (b, r, top[:, 0])
            elif c == A.TIE:
                assert ((top[:, :2] - 0.5).abs() <= 1e-9).all(), (b, r, top[:, :2])
            elif c in (A.RAMPUP, A.RAMPDOWN):
                tmax = torch.stack([s[:, r, t:t + 64].max(-1).values for t in range(0, ln, 64)], -1)       # [H, tiles]
                if c == A.RAMPDOWN:
                    assert (tmax.argmax(-1) == 0).all()
                    assert (s[:, r].argmax(-1) < 64).all()
                else:
                    nfull = ln // 64
                    d = tmax[:, 1:] - tmax[:, :-1]
                    assert (d[:, :max(nfull - 1, 0)] >= 10).all(), (b, r, d)          # full tile to full tile: 16 nats
                    if ln % 64 and ln > 64:                                           # ragged last tile of n keys: 0.25 n nats, still a rise
                        assert (d[:, -1] >= 0.25 * (ln % 64) - 2.0).all() and (d[:, -1] > -1.0).all(), (b, r, d)
            elif c == A.SHIFTED:
                assert (lse[b, :, r].abs() >= 70).all(), (b, r, lse[b, :, r])
    assert (lse[h.cls[:, None, :].expand(B, H, Sq) == A.SHIFTED].abs() >= 70).all()
    ov = o.view(B, Sq, -1)
    for c in present:
        sel = h.cls == c
        assert ov[sel].norm() / ov[sel].numel() ** 0.5 > 0.02, A.CLASSES[c]


def test_fused_passes_share_one_key_plan():
    """the second geometry of test_cross_attn_fused_gpu.CASES: three ranged caption groups and an unranged pass over one K | V. Range
    (0, 200) ends where (200, 130) begins: each one's edge key is the other's intruder, and the rows keep their properties."""
    k, v, ps = A.make_passes(2, 330, 3, [(3, 32, [(0, 330), (0, 200), (200, 130)]), (1, 42, None)])
    assert any(pl["intr"] for pl in ps[0].plans)
    for h in ps:
        o, lse = A.ref(h.q, k, v, 2, kv_range=h.kv_range, bmod=3)
        P = [torch.softmax(_scores(h, 2, b)[0], -1).sort(-1, descending=True).values for b in range(h.q.shape[0])]
        top = torch.stack([p[:, :, :2] for p in P]).transpose(1, 2)               # [B, Sq, H, 2]
        assert (top[h.cls == A.PEAKED][..., 0] >= 1 - 1e-9).all()
        assert ((top[h.cls == A.TIE] - 0.5).abs() <= 1e-9).all()
        assert (lse.transpose(1, 2)[h.cls == A.SHIFTED].abs() >= 70).all()
        assert len(set(h.cls.reshape(-1).tolist())) >= 6
    h = ps[0]
    sel = h.cls == A.INTRUDER
    o, _ = A.ref(h.q, k, v, 2, kv_range=h.kv_range, bmod=3)
    o_all, _ = A.ref(h.q, k, v, 2, bmod=3)
    assert sel.any() and ((o_all[sel] - o[sel]).norm() / o[sel].norm()).item() >= 0.5


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[4]], ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_intruder_rows_depend_on_the_range(shape):
    """ignoring kv_range (every row sees the whole buffer) changes the intruder rows' output by a relative L2 of >= 0.5"""
    B, H, Sq, Skv, ranges, bmod = shape
    h = A.make(B, H, Sq, Skv, ranges, bmod)
    sel = h.cls == A.INTRUDER
    assert sel.any()
    o, _ = A.ref(h.q, h.k, h.v, H, kv_range=h.kv_range, bmod=bmod)
    o_all, _ = A.ref(h.q, h.k, h.v, H, kv_range=None, bmod=bmod)
    assert ((o_all[sel] - o[sel]).norm() / o[sel].norm()).item() >= 0.5
    others = ~sel & (h.cls != A.BENIGN)          # and the range matters to the other rows of the ranged groups as well
    assert (o_all[others] - o[others]).norm() > 0


@pytest.mark.parametrize("shape", [s for s in SHAPES if not s[5] and s[0] * s[2] >= 7],
                         ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_intruder_rows_depend_on_the_blocked_mask(shape):
    """ignoring the `blocked` mask changes the intruder rows' output by a relative L2 of >= 0.5; the mask has rows whose leading tiles are
    closed, rows that are closed everywhere and rows with an open head and a closed tail"""
    B, H, Sq, Skv, ranges, bmod = shape
    h = A.make(B, H, Sq, Skv)
    m = A.masks(B, Sq, Skv, "blocked", hard=h)
    sel = (h.cls == A.INTRUDER) & ~(m == -10000.0).all(-1)
    assert sel.any()
    o, _ = A.ref(h.q, h.k, h.v, H, mask=m)
    o_open, _ = A.ref(h.q, h.k, h.v, H)
    assert ((o_open[sel] - o[sel]).norm() / o[sel].norm()).item() >= 0.5
    closed = m == -10000.0
    assert closed.all(-1).any() and (closed[:, :, 0] & ~closed[:, :, -1]).any() and (~closed[:, :, 0] & closed[:, :, -1]).any()
    assert torch.isfinite(o).all()


def test_generated_values_are_bf16_exact_and_peaked_and_tie_targets_are_disjoint():
    h = A.make(4, 2, 48, 200, RANGES2, 2)
    for t in (h.q, h.k, h.v, h.dout):
        assert torch.equal(t, t.bfloat16().float())
    for pl in h.plans:
        tie = set(pl["tie"][:2]) if pl["tie"] else set()
        assert not tie & {j for j, _ in pl["peaked"]} and not tie & {j for j, _ in pl["intr"]}
    assert A.peaked_locals(200) == [0, 63, 64, 199, 100] and A.peaked_locals(33) == [0, 32, 16]


def test_fp32_reference_error_is_what_the_tolerances_assume():
    """plain fp32 evaluation against fp64 on (2, 2, 70, 130): benign rows at the few-e-7 of the other tests, shifted rows (|s| ~ 80, ulp 8e-6)
    an order and a half above -- the reason the fp32 bounds of the GPU tests are max(project tolerance, 4 x this error)"""
    h = A.make(2, 2, 70, 130)
    r64 = A.grads(h.q, h.k, h.v, h.dout, 2)
    r32 = A.grads(h.q, h.k, h.v, h.dout, 2, dtype=torch.float32)
    err = lambda c: ((r32["o"][h.cls == c].double() - r64["o"][h.cls == c]).norm() / r64["o"][h.cls == c].norm()).item()
    assert err(A.BENIGN) < 1e-6 and 3e-6 < err(A.SHIFTED) < 1e-4
    assert (r32["lse"].double() - r64["lse"]).abs().max().item() < 5e-5


@pytest.mark.parametrize("geo,mask,p", [((2, 2, 70, 130, None, 0), "blocked", 0.0), ((4, 2, 48, 200, RANGES2, 2), "none", 0.0),
                                        ((2, 2, 33, 33, None, 0), "dense", 0.1)])
def test_backward_from_the_stored_lse_is_the_autograd_gradient(geo, mask, p):
    """grads_lse (P = exp(s - lse), delta = rowsum(dO * O)) and grads (autograd) agree in fp64: the fp32 yardstick measures rounding only"""
    import dropout_ref as R
    B, H, Sq, Skv, ranges, bmod = geo
    h = A.make(B, H, Sq, Skv, ranges, bmod)
    keep = torch.from_numpy(R.attn_keep(5, 9, B, H, Sq, Skv, p)) if p else None
    kw = dict(mask=A.masks(B, Sq, Skv, mask, hard=h), kv_range=h.kv_range, bmod=bmod, keep=keep, p=p)
    a, b = A.grads(h.q, h.k, h.v, h.dout, H, **kw), A.grads_lse(h.q, h.k, h.v, h.dout, H, dtype=torch.float64, **kw)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert (a[n] - b[n]).norm() <= 1e-10 * a[n].norm(), n


def test_window_backward_from_the_stored_lse_is_the_autograd_gradient():
    g = torch.Generator().manual_seed(3)
    N, nW, heads = 98, 2, 2
    rowmap, rel = torch.randperm(nW * N, generator=g), torch.randint(0, 500, (N, N), generator=g)
    label = torch.randint(0, 3, (nW * N,), generator=g).to(torch.uint8)
    w = A.make_window(2, heads, rowmap, nW, N, 500)
    a = A.grads_window(w.qkv, w.table, w.dout, heads, rowmap, label, rel, nW, N)
    b = A.grads_window(w.qkv, w.table, w.dout, heads, rowmap, label, rel, nW, N, via_lse=True)
    for n in ("o", "lse", "dqkv", "dtable"):
        assert (a[n] - b[n]).norm() <= 1e-10 * a[n].norm(), n


@pytest.mark.parametrize("N,nW", [(98, 1), (196, 2), (392, 1)])
def test_window_classes(N, nW):
    """make_window on an identity row map with a full relative-position index: peaked rows one-hot, tie rows on two keys, shifted rows |lse|
    >= 70 -- with the +-20 bias table applied -- and the bias decides the maximum of most benign rows"""
    heads, B = 2, 1
    g = torch.Generator().manual_seed(N)
    rowmap = torch.arange(nW * N)
    rel = torch.randint(0, 500, (N, N), generator=g)
    w = A.make_window(B, heads, rowmap, nW, N, 500)
    o, lse = A.ref_window(w.qkv, w.table, heads, rowmap, None, rel, nW, N)
    o0, _ = A.ref_window(w.qkv, torch.zeros_like(w.table), heads, rowmap, None, rel, nW, N)
    C = heads * 32
    x = w.qkv.double()[:, rowmap].reshape(nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s = (x[0] * 32 ** -0.5) @ x[1].transpose(-2, -1)
    sb = s + w.table.double()[rel.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)[None]
    top = torch.softmax(sb, -1).sort(-1, descending=True).values                     # [nW, heads, N, N]
    cls = w.cls[0].view(nW, 1, N).expand(nW, heads, N)
    assert (top[..., 0][cls == 1] >= 1 - 1e-9).all()
    assert (top[..., :2].sum(-1)[cls == 2] >= 1 - 1e-9).all() and (top[..., 1][cls == 2] > 1e-18).all()
    assert (lse[cls == 3].abs() >= 70).all()
    moved = (sb.argmax(-1) != s.argmax(-1))[cls == 0].float().mean().item()
    assert moved > 0.5, moved
    assert (o - o0)[0][w.cls[0] == 0].norm() / o[0][w.cls[0] == 0].norm() > 0.5
    for c in range(4):
        sel = w.cls[0] == c
        assert sel.any() and o[0][sel].norm() / o[0][sel].numel() ** 0.5 > 0.02
