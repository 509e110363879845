"""Hard inputs for the attention kernels, and the explicit references they are held against (a plain module like dropout_ref.py).

The other attention tests draw q and k as randn * 0.7 ... 1.5 with scale 1/8: scaled scores stay within a few nats and the running
maximum of the online softmax moves by fractions of a nat from key tile to key tile. make() builds rows of seven classes that cycle
with the row index (class = (b * Sq + row + first) % 7, so every 16-row sub-tile holds several):

  benign    as in the other tests
  peaked    one key dominates (45.75 nats against +-20): P is one-hot. The dominant keys sit at local positions 0, 63, 64, len - 1 and
            len // 2 of the keys the row may see (first / last lane of a tile, a tile boundary, the ragged tail)
  tie       two keys, a tile apart where the range allows, share the maximum exactly, the others are far below: P = 1/2, 1/2
  rampup    the score grows by 0.25 nat per key: every 64-key tile raises the running maximum by 16 nats (the rescale exp(m_old - m_new)
            underflows from tile to tile)
  rampdown  the score falls by 0.25 nat per key: the maximum is in tile 0 and never moves, the later tiles underflow
  shifted   every score of the row carries a common offset of +-80 nats (|lse| ~ 80: the lse * log2(e) re-use of the backward kernels)
  intruder  a key the row may NOT see -- the buffer row just before / after its kv_range (intruder="range") or a key that the
            `blocked` mask closes (intruder="mask") -- would score ~61 nats above everything visible

Construction (head_dim 64, scale 1/8; every value is exactly representable in bf16, so fp32 kernels, bf16 kernels and the references
read identical numbers). Key j of the buffer: dim 0 = j // 16, dim 1 = j % 16, dim 2 = 1, dims 3..63 = randn * 0.8 -- except on
"special" keys (peaked / tie targets, intruders) where dims 3..63 are a +-1 sign vector: a row of the 64 x 64 Sylvester-Hadamard matrix cut
to 61 columns, so two different special keys correlate by at most 3 / 61. Query rows: dims 0..2 are zero, dims 3..63 = randn * 0.8, then
  peaked / tie   dims 3..63 = 6 * sign vector of the target (score 6 * 61 / 8 = 45.75; both keys of a tie pair carry the same vector)
  rampup / down  dim 0 = +-32, dim 1 = +-2 (score +-0.25 j), the noise dims scaled by 0.25
  shifted        dim 2 = +-640
  intruder       dims 3..63 += 8 * sign vector of the intruder key (61 nats)
Targets are planned per K/V batch over ALL key ranges that read it (intruders first, then peaked targets, then tie pairs, a key has one
role), so peaked and tie target sets are disjoint. A class that a shape cannot hold (no key outside the range, fewer than 8 visible
keys for a tie) falls back to benign in the class vector.

masks() builds additive fp32 masks with ordinary finite values (`dense`, `dense1`) or closed regions whose position matters (`blocked`);
ref() is explicit fp64 softmax attention returning o and lse, ref_fp32() the same formula in plain fp32 torch (the yardstick of the
fp32 tolerances), grads() either of them with dq / dk / dv by autograd, grads_lse() the backward from the stored lse (the fp32 yardstick
of the gradients). make_window() / ref_window() / grads_window() do the same for the 3-D window attention (head_dim 32, classes placed by
window slot)."""
import types

import torch

CLASSES = ("benign", "peaked", "tie", "rampup", "rampdown", "shifted", "intruder")
BENIGN, PEAKED, TIE, RAMPUP, RAMPDOWN, SHIFTED, INTRUDER = range(7)
PEAK_AMP, INTRUDER_AMP, SHIFT_AMP = 6.0, 8.0, 640.0


def _hadamard(n):
    h = torch.ones((1, 1))
    while h.shape[0] < n:
        h = torch.cat((torch.cat((h, h), 1), torch.cat((h, -h), 1)), 0)
    return h


def _bf16(t):
    return t.bfloat16().float()


def peaked_locals(ln):
    """local positions of the dominant keys of peaked rows among `ln` visible keys"""
    out = []
    for j in (0, 63, 64, ln - 1, ln // 2):
        j = min(max(j, 0), ln - 1)
        if j not in out:
            out.append(j)
    return out


def plan_keys(Skv, ranges, intruder):
    """roles of the keys of one K/V buffer read through `ranges` [(start, len)]: per range dict(peaked=[(key, vec)], tie=(key a, key b, vec)
    | None, intr=[(key, vec)]) with BUFFER key indices and sign vector ids >= 1; plus the map key -> vector id of every special key"""
    used, plans, nvec = {}, [dict(peaked=[], tie=None, intr=[]) for _ in ranges], [0]

    def new_vec():
        nvec[0] += 1
        assert nvec[0] <= 63, "more special keys than sign vectors"
        return nvec[0]

    for pl, (s0, ln) in zip(plans, ranges):
        if intruder == "range":
            cands = [j for j in (s0 - 1, s0 + ln) if 0 <= j < Skv]
        elif intruder == "mask":
            cands = [s0 + ln // 3] if ln >= 6 else []
        else:
            cands = []
        vec = None
        for j in cands:
            if j not in used:
                vec = vec or new_vec()
                used[j] = ("intr", vec)
                pl["intr"].append((j, vec))
    for pl, (s0, ln) in zip(plans, ranges):
        for loc in peaked_locals(ln):
            j = s0 + loc
            if j not in used:
                used[j] = ("peaked", new_vec())
            if used[j][0] == "peaked":
                pl["peaked"].append((j, used[j][1]))
    for pl, (s0, ln) in zip(plans, ranges):
        if ln < 8:
            continue
        a = next(j for j in range(s0 + 1, s0 + ln) if j not in used)
        b = next(j for j in range(s0 + ln - 2, s0, -1) if j not in used)
        if b > a:
            vec = new_vec()
            used[a] = used[b] = ("tie", vec)
            pl["tie"] = (a, b, vec)
    return plans, {j: v for j, (_, v) in used.items()}


def _vec_rows(H, hd):
    """[H, 64, hd - 3]: sign vector of id v for head h (another row of the Hadamard matrix per head; row 0, all ones, is never used)"""
    had = _hadamard(64)[:, :hd - 3]
    ids = torch.arange(64)
    return torch.stack([had[(ids - 1 + 5 * h) % 63 + 1] for h in range(H)])


def build_kv(Bkv, H, Skv, vecs, g, head_dim=64):
    """k, v [Bkv, Skv, H * head_dim] fp32 holding bf16-exact values; vecs: key -> sign vector id (plan_keys)"""
    hd = head_dim
    k = torch.zeros((Bkv, Skv, H, hd))
    j = torch.arange(Skv)
    k[:, :, :, 0] = (j // 16).float()[None, :, None]
    k[:, :, :, 1] = (j % 16).float()[None, :, None]
    k[:, :, :, 2] = 1.0
    k[:, :, :, 3:] = torch.randn((Bkv, Skv, H, hd - 3), generator=g) * 0.8
    rows = _vec_rows(H, hd)
    for key, vec in vecs.items():
        k[:, key, :, 3:] = rows[:, vec][None]
    v = torch.randn((Bkv, Skv, H * hd), generator=g) * 0.8
    return _bf16(k.reshape(Bkv, Skv, H * hd)), _bf16(v)


def build_q(B, H, Sq, plan_of_batch, g, first=0, head_dim=64):
    """q, dout [B, Sq, H * head_dim] and the class vector [B, Sq]; plan_of_batch(b) -> the plan (plan_keys) of the range batch b reads"""
    hd = head_dim
    q = torch.zeros((B, Sq, H, hd))
    q[:, :, :, 3:] = torch.randn((B, Sq, H, hd - 3), generator=g) * 0.8
    q = _bf16(q)
    rows = _vec_rows(H, hd)
    cls = torch.zeros((B, Sq), dtype=torch.int64)
    for b in range(B):
        pl = plan_of_batch(b)
        for r in range(Sq):
            n = b * Sq + r + first
            c, occ = n % 7, n // 7
            if (c == TIE and pl["tie"] is None) or (c == INTRUDER and not pl["intr"]) or (c == PEAKED and not pl["peaked"]):
                c = BENIGN
            cls[b, r] = c
            if c == PEAKED:
                q[b, r, :, 3:] = PEAK_AMP * rows[:, pl["peaked"][occ % len(pl["peaked"])][1]]
            elif c == TIE:
                q[b, r, :, 3:] = PEAK_AMP * rows[:, pl["tie"][2]]
            elif c in (RAMPUP, RAMPDOWN):
                sgn = 1.0 if c == RAMPUP else -1.0
                q[b, r, :, 0], q[b, r, :, 1] = 32.0 * sgn, 2.0 * sgn
                q[b, r, :, 3:] *= 0.25
            elif c == SHIFTED:
                q[b, r, :, 2] = SHIFT_AMP if occ % 2 == 0 else -SHIFT_AMP
            elif c == INTRUDER:
                q[b, r, :, 3:] += INTRUDER_AMP * rows[:, pl["intr"][0][1]]
    dout = torch.randn((B, Sq, H * hd), generator=g)
    return _bf16(q.reshape(B, Sq, H * hd)), _bf16(dout), cls


def make(B, H, Sq, Skv, ranges=None, bmod=0, head_dim=64, seed=0, intruder="auto", first=0):
    """One launch geometry as valor_attn_fwd takes it: B query batches of Sq rows, K/V batch b % bmod (bmod = 0: b), `ranges` [(start, len)]
    per query GROUP b // bmod. intruder: "range" | "mask" | None ("auto": "range" when ranges are given, else "mask").
    Returns a namespace: q, dout [B, Sq, E], k, v [Bkv, Skv, E] (fp32 tensors of bf16-exact values), cls [B, Sq] (index into CLASSES),
    kv_range int32 [B, 2] | None, intr_local [B] (local index of the intruder key a `blocked` mask closes, -1: none), plans."""
    assert head_dim == 64, "the construction is worked out for head_dim 64 and scale 1/8 (make_window: head_dim 32)"
    if intruder == "auto":
        intruder = "range" if ranges is not None else "mask"
    g = torch.Generator().manual_seed(seed * 7919 + B * 1000003 + H * 10007 + Sq * 101 + Skv)
    rl = list(ranges) if ranges is not None else [(0, Skv)]
    plans, vecs = plan_keys(Skv, rl, intruder)
    Bkv = bmod if bmod > 0 else B
    k, v = build_kv(Bkv, H, Skv, vecs, g, head_dim)
    grp = (lambda b: b // bmod) if ranges is not None else (lambda b: 0)
    q, dout, cls = build_q(B, H, Sq, lambda b: plans[grp(b)], g, first, head_dim)
    kvr = torch.tensor([list(rl[grp(b)]) for b in range(B)], dtype=torch.int32) if ranges is not None else None
    intr_local = torch.full((B,), -1, dtype=torch.int64)
    if intruder == "mask":
        for b in range(B):
            pl = plans[grp(b)]
            if pl["intr"]:
                intr_local[b] = pl["intr"][0][0] - rl[grp(b)][0]
    return types.SimpleNamespace(q=q, k=k, v=v, dout=dout, cls=cls, kv_range=kvr, bmod=bmod, H=H, intr_local=intr_local, plans=plans,
                                 ranges=rl, intruder=intruder)


def make_passes(H, Skv, bmod, passes, seed=0):
    """Several decoder passes over ONE K | V (the fused two-pass cross-attention): passes = [(groups, T, ranges per group | None)], pass i has
    groups * bmod query batches of T rows. The key roles are planned over the ranges of all passes together.
    Returns k, v [bmod, Skv, E] and one namespace per pass (q, dout, cls, kv_range, bmod, H, plans, ranges)."""
    g = torch.Generator().manual_seed(seed * 7919 + bmod * 1000003 + H * 10007 + Skv)
    rls = [list(r) if r is not None else [(0, Skv)] for _, _, r in passes]
    plans, vecs = plan_keys(Skv, [r for rl in rls for r in rl], "range")
    k, v = build_kv(bmod, H, Skv, vecs, g)
    out, at = [], 0
    for i, ((G, T, ranges), rl) in enumerate(zip(passes, rls)):
        mine = plans[at:at + len(rl)]
        at += len(rl)
        B = G * bmod
        grp = (lambda b: b // bmod) if ranges is not None else (lambda b: 0)
        q, dout, cls = build_q(B, H, T, lambda b: mine[grp(b)], g, first=3 * i)
        kvr = torch.tensor([list(rl[grp(b)]) for b in range(B)], dtype=torch.int32) if ranges is not None else None
        out.append(types.SimpleNamespace(q=q, k=k, v=v, dout=dout, cls=cls, kv_range=kvr, bmod=bmod, H=H, plans=mine, ranges=rl))
    return k, v, out


def masks(B, Sq, Skv, kind, hard=None, seed=0):
    """additive fp32 masks [B | 1, Sq, Skv]: "dense" N(0, 3) per (b, q, key); "dense1" the same with one batch (the broadcast path, mask_bs = 0);
    "blocked": -10000 on a leading block of whole 64-key tiles (half of the keys when Skv <= 64) for every third row, on every key for every
    fifth row, on the last Skv // 8 keys in odd batches, and (hard given) on the intruder key of the intruder rows. None for "none"."""
    if kind in (None, "none"):
        return None
    g = torch.Generator().manual_seed(seed * 31 + B * 7 + Sq * 1009 + Skv)
    if kind == "dense":
        return torch.randn((B, Sq, Skv), generator=g) * 3.0
    if kind == "dense1":
        return torch.randn((1, Sq, Skv), generator=g) * 3.0
    assert kind == "blocked", kind
    m = torch.zeros((B, Sq, Skv))
    nt = (Skv - 1) // 64                   # whole tiles ahead of the last one
    for b in range(B):
        if b % 2 == 1:
            m[b, :, Skv - max(1, Skv // 8):] = -10000.0
        for r in range(Sq):
            n = b * Sq + r
            if n % 3 == 1:
                m[b, r, :(64 * (1 + (n // 3) % nt) if nt > 0 else Skv // 2)] = -10000.0
            if n % 5 == 2:
                m[b, r, :] = -10000.0
            if hard is not None and hard.cls[b, r] == INTRUDER and hard.intr_local[b] >= 0:
                m[b, r, hard.intr_local[b]] = -10000.0
    return m


def ref(q, k, v, H, mask=None, kv_range=None, bmod=0, scale=0.125, keep=None, p=0.0, dtype=torch.float64, head_dim=64):
    """Explicit softmax attention in `dtype`: q [B, Sq, E], k / v [Bkv, Skv, E], mask additive [B | 1, Sq, >= len] indexed by the LOCAL key,
    kv_range [B, 2] (start, len), query batch b reads K/V batch b % bmod (bmod = 0: b); keep: bool [B, H, Sq, Skv] with dropout p
    (tests/dropout_ref.py). Returns o [B, Sq, E] and lse [B, H, Sq] (of the undropped scores)."""
    B, Sq, E = q.shape
    hd = head_dim
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    outs, lses = [], []
    for b in range(B):
        kb = b % bmod if bmod > 0 else b
        s0, ln = (0, k.shape[1]) if kv_range is None else (int(kv_range[b][0]), int(kv_range[b][1]))
        qq = q[b].view(Sq, H, hd).transpose(0, 1)
        kk = k[kb, s0:s0 + ln].view(ln, H, hd).transpose(0, 1)
        vv = v[kb, s0:s0 + ln].view(ln, H, hd).transpose(0, 1)
        s = qq @ kk.transpose(1, 2) * scale
        if mask is not None:
            s = s + mask[b if mask.shape[0] > 1 else 0, :, :ln].to(dtype)
        m = s.max(-1, keepdim=True).values.detach()
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        pr = e / l
        if keep is not None:
            pr = pr * keep[b, :, :, :ln].to(dtype) * (1.0 / (1.0 - p))
        outs.append((pr @ vv).transpose(0, 1).reshape(Sq, E))
        lses.append((m + torch.log(l)).squeeze(-1))
    return torch.stack(outs), torch.stack(lses)


def ref_fp32(*a, **kw):
    """the same formula evaluated in plain fp32 torch"""
    return ref(*a, dtype=torch.float32, **kw)


def grads(q, k, v, dout, H, dtype=torch.float64, **kw):
    """dict(o, lse, dq, dk, dv) of ref() in `dtype`, the gradients of sum(o * dout) by autograd"""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    o, lse = ref(q, k, v, H, dtype=dtype, **kw)
    (o * dout.to(dtype)).sum().backward()
    return dict(o=o.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def grads_lse(q, k, v, dout, H, mask=None, kv_range=None, bmod=0, scale=0.125, keep=None, p=0.0, dtype=torch.float32, head_dim=64):
    """The fp32 yardstick of the gradients: dict(o, lse, dq, dk, dv) with o and lse as ref() gives them in `dtype` and the backward
    evaluated the way the C ABI makes every kernel evaluate it -- from the STORED o and lse:
        P = exp(s - lse), delta = rowsum(dO * O), dP = dO V^T (* keep / (1 - p)), dS = P * (dP - delta),
        dQ = scale dS K, dK = scale dS^T Q, dV = (P * keep / (1 - p))^T dO
    so the rounding of lse as one number of `dtype` (ulp 8e-6 at 80 nats, 1e-3 on a row whose every key carries -10000) reaches P as it
    does in any implementation of that interface. In exact arithmetic this is the gradient autograd gives (grads(); held together in fp64
    by tests/test_attn_hard_inputs_cpu.py)."""
    B, Sq, E = q.shape
    hd = head_dim
    q, k, v, dout = q.to(dtype), k.to(dtype), v.to(dtype), dout.to(dtype)
    o, lse = ref(q, k, v, H, mask=mask, kv_range=kv_range, bmod=bmod, scale=scale, keep=keep, p=p, dtype=dtype, head_dim=hd)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    ks = 1.0 / (1.0 - p) if keep is not None else 1.0
    for b in range(B):
        kb = b % bmod if bmod > 0 else b
        s0, ln = (0, k.shape[1]) if kv_range is None else (int(kv_range[b][0]), int(kv_range[b][1]))
        qq = q[b].view(Sq, H, hd).transpose(0, 1)
        kk = k[kb, s0:s0 + ln].view(ln, H, hd).transpose(0, 1)
        vv = v[kb, s0:s0 + ln].view(ln, H, hd).transpose(0, 1)
        do = dout[b].view(Sq, H, hd).transpose(0, 1)
        s = qq @ kk.transpose(1, 2) * scale
        if mask is not None:
            s = s + mask[b if mask.shape[0] > 1 else 0, :, :ln].to(dtype)
        pr = torch.exp(s - lse[b][:, :, None])
        dp = do @ vv.transpose(1, 2)
        pd = pr
        if keep is not None:
            kp = keep[b, :, :, :ln].to(dtype) * ks
            dp, pd = dp * kp, pr * kp
        delta = (do * o[b].view(Sq, H, hd).transpose(0, 1)).sum(-1, keepdim=True)
        ds = pr * (dp - delta)
        dq[b] = ((ds @ kk) * scale).transpose(0, 1).reshape(Sq, E)
        dk[kb, s0:s0 + ln] += ((ds.transpose(1, 2) @ qq) * scale).transpose(0, 1).reshape(ln, E)
        dv[kb, s0:s0 + ln] += (pd.transpose(1, 2) @ do).transpose(0, 1).reshape(ln, E)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


# ---------------------------------------------------------------------------------------------- window attention (head_dim 32)
WIN_CLASSES = ("benign", "peaked", "tie", "shifted")
WIN_PEAK_AMP, WIN_SHIFT_AMP = 24.0, 576.0


def make_window(B, heads, rowmap, nW, N, table_rows, seed=0):
    """Hard rows for valor_win_attn_fwd / bwd. rowmap: int64 [nW * N], row of a sample held by slot n of window w (the geometry's map).
    Classes by window slot, class = (w + n) % 4 over WIN_CLASSES. head_dim 32, scale 32^-0.5: key dim 0 = 1, dim 1 = (n % 16) / 8 (so the
    two keys of a tie pair differ and a tie row's dQ is not identically zero), dims 2..31 = randn * 0.5, or a +-1 vector (Hadamard 32 cut
    to 30 columns) on the target slots peaked_locals(N) and the tie pair (1, N - 2 moved off the peaked slots); peaked / tie queries =
    24 * that vector (127 nats against ~+-47 of the others, so a bias of +-20 cannot turn them; the bias splits the tie); shifted queries
    carry +-576 in dim 0 (+-102 nats, at least 70 with the bias against them). The bias table is randn * 0.5 with every eighth entry +-20: on
    benign rows the bias decides the maximum. Returns a namespace: qkv [B, rows, 3C], dout [B, rows, C], table [table_rows, heads], cls [B, rows]."""
    g = torch.Generator().manual_seed(seed * 7919 + B * 1000003 + nW * 10007 + N)
    C, rows = heads * 32, nW * N
    had = _hadamard(32)[:, :30]
    q = torch.zeros((B, rows, heads, 32))
    k = torch.zeros((B, rows, heads, 32))
    q[..., 1:] = torch.randn((B, rows, heads, 31), generator=g) * 0.8
    k[..., 2:] = torch.randn((B, rows, heads, 30), generator=g) * 0.5
    k[..., 0] = 1.0
    v = torch.randn((B, rows, heads, 32), generator=g) * 0.8
    peaked = peaked_locals(N)
    a = next(j for j in range(1, N) if j not in peaked)
    b_ = next(j for j in range(N - 2, 0, -1) if j not in peaked)
    vec_of = {j: 1 + i for i, j in enumerate(peaked)}
    tie_vec = len(peaked) + 1
    cls = torch.zeros((B, rows), dtype=torch.int64)
    rm = rowmap.view(nW, N)
    for w in range(nW):
        k[:, rm[w], :, 1] = ((torch.arange(N) % 16).float() / 8.0)[None, :, None]
        for j, vec in list(vec_of.items()) + ([(a, tie_vec), (b_, tie_vec)] if b_ > a else []):
            for h in range(heads):
                k[:, rm[w, j], h, 2:] = had[(vec - 1 + 5 * h) % 31 + 1]
        for n in range(N):
            r, c, occ = rm[w, n], (w + n) % 4, (w + n) // 4
            if c == 2 and not b_ > a:
                c = 0
            cls[:, r] = c
            if c in (1, 2):
                vec = vec_of[peaked[occ % len(peaked)]] if c == 1 else tie_vec
                q[:, r, :, 1] = 0.0
                for h in range(heads):
                    q[:, r, h, 2:] = WIN_PEAK_AMP * had[(vec - 1 + 5 * h) % 31 + 1]
            elif c == 3:
                q[:, r, :, 0] = WIN_SHIFT_AMP if occ % 2 == 0 else -WIN_SHIFT_AMP
    table = torch.randn((table_rows, heads), generator=g) * 0.5
    big = torch.arange(table_rows) % 8 == 3
    table[big] = torch.where(torch.rand((int(big.sum()), heads), generator=g) < 0.5, -20.0, 20.0)
    qkv = torch.cat((q.reshape(B, rows, C), k.reshape(B, rows, C), v.reshape(B, rows, C)), -1)
    dout = torch.randn((B, rows, C), generator=g)
    return types.SimpleNamespace(qkv=_bf16(qkv), dout=_bf16(dout), table=_bf16(table), cls=cls)


def ref_window(qkv, table, heads, rowmap, label, rel_index, nW, N, dtype=torch.float64):
    """Explicit window attention: qkv [B, rows, 3C] (q | k | v, C = heads * 32), rowmap int64 [nW * N], label uint8 [nW * N] | None (keys whose
    region label differs from the query's get -100), rel_index int64 [N, N] into the bias table [., heads].
    Returns o [B, rows, C] and lse [B * nW, heads, N]."""
    B, rows, C3 = qkv.shape
    C = C3 // 3
    xw = qkv.to(dtype)[:, rowmap].reshape(B * nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    q, k, v = xw[0], xw[1], xw[2]
    s = (q * 32 ** -0.5) @ k.transpose(-2, -1)
    s = s + table.to(dtype)[rel_index.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)[None]
    if label is not None:
        lab = label.view(nW, N).long()
        m = torch.where(lab[:, None, :] != lab[:, :, None], -100.0, 0.0).to(dtype)
        s = (s.view(B, nW, heads, N, N) + m[None, :, None]).view(B * nW, heads, N, N)
    mx = s.max(-1, keepdim=True).values.detach()
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    ow = ((e / l) @ v).transpose(1, 2).reshape(B, nW * N, C)
    o = torch.empty((B, rows, C), dtype=dtype).index_copy(1, rowmap, ow)
    return o, (mx + torch.log(l)).squeeze(-1)


def grads_window(qkv, table, dout, heads, rowmap, label, rel_index, nW, N, dtype=torch.float64, via_lse=False):
    """dict(o, lse, dqkv, dtable) of ref_window() in `dtype`: by autograd, or (via_lse: the fp32 yardstick, see grads_lse) by the explicit
    backward from the stored o and lse, P = exp(s - lse)"""
    B, rows, C3 = qkv.shape
    C = C3 // 3
    if not via_lse:
        x, t = qkv.detach().to(dtype).requires_grad_(True), table.detach().to(dtype).requires_grad_(True)
        o, lse = ref_window(x, t, heads, rowmap, label, rel_index, nW, N, dtype=dtype)
        (o * dout.to(dtype)).sum().backward()
        return dict(o=o.detach(), lse=lse.detach(), dqkv=x.grad, dtable=t.grad)
    o, lse = ref_window(qkv, table, heads, rowmap, label, rel_index, nW, N, dtype=dtype)
    xw = qkv.to(dtype)[:, rowmap].reshape(B * nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    q, k, v = xw[0], xw[1], xw[2]
    s = (q * 32 ** -0.5) @ k.transpose(-2, -1)
    s = s + table.to(dtype)[rel_index.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)[None]
    if label is not None:
        lab = label.view(nW, N).long()
        m = torch.where(lab[:, None, :] != lab[:, :, None], -100.0, 0.0).to(dtype)
        s = (s.view(B, nW, heads, N, N) + m[None, :, None]).view(B * nW, heads, N, N)
    win = lambda t: t.to(dtype)[:, rowmap].reshape(B * nW, N, heads, 32).transpose(1, 2)
    do, ow = win(dout), win(o)
    pr = torch.exp(s - lse[..., None])
    ds = pr * (do @ v.transpose(-2, -1) - (do * ow).sum(-1, keepdim=True))
    dq, dk, dv = (ds @ k) * 32 ** -0.5, (ds.transpose(-2, -1) @ q) * 32 ** -0.5, pr.transpose(-2, -1) @ do
    unwin = lambda t: t.transpose(1, 2).reshape(B, nW * N, C)
    dqkv = torch.empty((B, rows, C3), dtype=dtype).index_copy(1, rowmap, torch.cat((unwin(dq), unwin(dk), unwin(dv)), -1))
    dtable = torch.zeros(table.shape, dtype=dtype).index_add(0, rel_index.reshape(-1), ds.sum(0).permute(1, 2, 0).reshape(N * N, heads))
    return dict(o=o, lse=lse, dqkv=dqkv, dtable=dtable)
