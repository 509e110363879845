"""Host restatement of the two dropout mask laws and fp64 references that take a keep mask.

Attention (valor_amd/csrc/attn_common.h): a 32-bit hash per probability, keyed per (batch, head):
    hk   = attn_drop_headkey(seed, offset, b * H + h)
    bits = attn_drop_bits(hk, q * Skv + local_key)            local_key counts from the start of the batch's key range, the pitch is
                                                              the Skv ARGUMENT of the launch (rows per K/V batch), never the range length
Fused LayerNorm (valor_amd/csrc/common.h, layernorm.hip): Philox4x32-10,
    bits = philox4x32_10(seed, offset + (row * cols + c) / 4)[c % 4]
In both `offset` is the full 64-bit sum of the by-value offset and the device-resident base (`rng_base`), and an element is KEPT iff
bits >= drop_threshold(p). The vectorised functions work on uint64 arrays with explicit 32-bit masks; the *_scalar functions are the
same laws written with Python ints (tests/test_dropout_ref_cpu.py holds the two against each other)."""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)
U24 = np.uint64(0xFFFFFF)
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def _u(x):
    return np.uint64(x)


# ---------------------------------------------------------------------------------------------- Philox4x32-10 (common.h)
def philox4x32_10(seed, ctr):
    """Philox4x32-10 of valor_amd/csrc/common.h (counter words 2-3 fixed), vectorised over a uint64 counter array -> 4 x uint64 words"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    c0, c1 = ctr & U32, ctr >> np.uint64(32)
    c2, c3 = np.full_like(ctr, 0x9E3779B9), np.full_like(ctr, 0xBB67AE85)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & U32, (k1 + np.uint64(0xBB67AE85)) & U32
    return c0, c1, c2, c3


def philox4x32_10_scalar(seed, ctr):
    """the same with Python ints: one counter -> a tuple of four 32-bit words"""
    k0, k1 = seed & M32, (seed >> 32) & M32
    c0, c1, c2, c3 = ctr & M32, (ctr >> 32) & M32, 0x9E3779B9, 0xBB67AE85
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def drop_threshold(p):
    """common.h drop_threshold: p arrives as a float32 and is widened to double; keep iff bits >= the result"""
    t = float(np.float32(p)) * 4294967296.0
    if t <= 0.0:
        return 0
    if t >= 4294967295.0:
        return 0xFFFFFFFF
    return int(t)


def keep_scale(p):
    """1 / (1 - p) of the float32 p the kernels receive"""
    return 1.0 / (1.0 - float(np.float32(p))) if p > 0 else 1.0


# ---------------------------------------------------------------------------------------------- attention hash (attn_common.h)
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & U32
    x = x ^ (x >> _u(16)); x = (x * _u(0x7FEB352D)) & U32
    x = x ^ (x >> _u(15)); x = (x * _u(0x846CA68B)) & U32
    return x ^ (x >> _u(16))


def attn_drop_headkey(seed, offset, head):
    """seed, offset: Python ints (64 bit); head: int array (b * H + h) -> uint64 array of 32-bit keys"""
    seed, offset = int(seed) & M64, int(offset) & M64
    head = np.asarray(head, dtype=np.uint64) & U32
    k = mix32((_u(offset & M32) + ((head * _u(0x9E3779B9)) & U32)) & U32)
    k = mix32(k ^ _u(offset >> 32) ^ _u(seed & M32))
    return mix32((k + _u(seed >> 32)) & U32)


def attn_drop_bits(hk, local):
    """__umul24: the low 24 bits of both operands, the low 32 bits of the product"""
    hk = np.asarray(hk, dtype=np.uint64)
    x = (np.asarray(local, dtype=np.uint64) & U32) ^ hk
    x = (((x & U24) * _u(0x9E3779)) + (hk >> _u(7))) & U32
    x = x ^ (x >> _u(15))
    x = (((x & U24) * _u(0x85EBCB)) + hk) & U32
    return x ^ (x >> _u(13))


def mix32_scalar(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def attn_drop_headkey_scalar(seed, offset, head):
    k = mix32_scalar(((offset & M32) + ((head & M32) * 0x9E3779B9 & M32)) & M32)
    k = mix32_scalar(k ^ ((offset >> 32) & M32) ^ (seed & M32))
    return mix32_scalar((k + ((seed >> 32) & M32)) & M32)


def attn_drop_bits_scalar(hk, local):
    x = (local & M32) ^ hk
    x = ((x & 0xFFFFFF) * 0x9E3779 + (hk >> 7)) & M32
    x ^= x >> 15
    x = ((x & 0xFFFFFF) * 0x85EBCB + hk) & M32
    return x ^ (x >> 13)


def attn_keep_heads(seed, offset, heads, Sq, Skv, p):
    """keep mask of the score matrices of the given head indices (b * H + h): bool [len(heads), Sq, Skv]"""
    hk = attn_drop_headkey(seed, offset, np.asarray(heads).reshape(-1))
    local = (np.arange(Sq, dtype=np.uint64)[:, None] * _u(Skv) + np.arange(Skv, dtype=np.uint64)[None, :])
    return attn_drop_bits(hk[:, None, None], local[None]) >= _u(drop_threshold(p))


def attn_keep(seed, offset, B, H, Sq, Skv, p, kv_range=None):
    """bool [B, H, Sq, Skv]: column j of batch b is LOCAL key j of that batch's key range (kv_range only says how many columns a batch
    uses: the element index is q * Skv + j whatever the range's start and length). offset = by-value offset + device base."""
    del kv_range
    return attn_keep_heads(seed, offset, np.arange(B * H), Sq, Skv, p).reshape(B, H, Sq, Skv)


# ---------------------------------------------------------------------------------------------- LayerNorm-side Philox mask
def ln_keep(seed, offset, rows, cols, p):
    """bool [rows, cols]: counter offset + (row * cols + c) / 4, word c % 4"""
    n = rows * cols
    ctr = _u(int(offset) & M64) + np.arange((n + 3) // 4, dtype=np.uint64)      # uint64 addition wraps like the device's
    w = philox4x32_10(int(seed) & M64, ctr)
    bits = np.stack(w, axis=1).reshape(-1)[:n]
    return (bits >= _u(drop_threshold(p))).reshape(rows, cols)


# ---------------------------------------------------------------------------------------------- fp64 references (torch)
def ref_attn_dropout(q, k, v, H, mask, kv_range, kv_bmod, scale, keep, p, want_lse=False):
    """O = (softmax(S + mask) * keep / (1 - p)) V per (batch, head), like tests/test_attention_gpu.py::_ref_attn.
    q [B, Sq, E], k / v [Bkv, Skv, E] fp64 (requires_grad for the gradients by autograd), keep: bool tensor [B, H, Sq, Skv] (or None).
    lse [B, H, Sq] is of the UNDROPPED scores."""
    import torch
    B, Sq, E = q.shape
    ks = keep_scale(p) if keep is not None else 1.0
    outs, lses = [], []
    for b in range(B):
        kb = b % kv_bmod if kv_bmod > 0 else b
        s0, ln = (0, k.shape[1]) if kv_range is None else (int(kv_range[b, 0]), int(kv_range[b, 1]))
        qq = q[b].view(Sq, H, 64).transpose(0, 1)
        kk = k[kb, s0:s0 + ln].view(ln, H, 64).transpose(0, 1)
        vv = v[kb, s0:s0 + ln].view(ln, H, 64).transpose(0, 1)
        s = qq @ kk.transpose(1, 2) * scale
        if mask is not None:
            s = s + mask[b if mask.shape[0] > 1 else 0, :, :ln].double()
        pr = torch.softmax(s, -1)
        if keep is not None:
            pr = pr * keep[b, :, :, :ln].to(pr.dtype) * ks
        outs.append((pr @ vv).transpose(0, 1).reshape(Sq, E))
        if want_lse:
            lses.append(torch.logsumexp(s, -1))
    o = torch.stack(outs)
    return (o, torch.stack(lses)) if want_lse else o


def ref_bdrln_dropout(x, bias, residual, gamma, beta, eps, keep, p, row_scale=None, rows_per_scale=0):
    """z = keep ? (x + bias) / (1 - p) : 0, then * row_scale[row // rows_per_scale], then + residual; y = LayerNorm(z). fp64 tensors
    (requires_grad for the gradients), keep: bool tensor [rows, cols] or None. Returns (z, y)."""
    import torch
    z = x if bias is None else x + bias
    if keep is not None:
        z = z * keep.to(z.dtype) * keep_scale(p)
    if row_scale is not None:
        rows = z.shape[0]
        z = z * row_scale.double()[torch.arange(rows, device=z.device) // rows_per_scale][:, None]
    if residual is not None:
        z = z + residual
    y = torch.nn.functional.layer_norm(z, (z.shape[-1],), gamma, beta, eps)
    return z, y
