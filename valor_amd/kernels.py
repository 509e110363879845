"""Tensor-level wrappers over the C-ABI (no autograd here; see ops.py).

torch is used for device memory, streams and shapes only; every computation below is a
HIP kernel in libvalor_hip.so. All tensors must live on the GPU: a CPU tensor is an error.
"""
import os

import torch

from . import lib
from .lib import ACT_NONE, DT_BF16, DT_F32, GEMM_PENDING_BYTES

_WS = {}
_WS_BYTES = 256 << 20
# device address of the 64-bit dropout counter every dropout launch adds to its by-value offset when it RUNS (include/valor_hip.h,
# `rng_base`); 0 = by-value windows only. Set by ops.DropoutState.enable_device_base().
RNG_BASE = 0


def dt_of(t):
    if t.dtype == torch.bfloat16:
        return DT_BF16
    if t.dtype == torch.float32:
        return DT_F32
    raise TypeError(f"valor_amd kernels support bf16 / fp32 only, got {t.dtype}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise lib.ValorHipError("valor_amd kernels need GPU tensors (no CPU fallback)")


def workspace(device, nbytes=_WS_BYTES):
    """Persistent fp32 scratch (split-K partials, column-sum partials)."""
    # one per (device, stream): two compute streams (valor_amd/streams.py) must not share split-K / column-sum partials
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        _WS[key] = ws
    return ws


def release_stream(stream):
    """forget the scratch that was allocated for `stream` (a graph-capture stream that is going away): its split-K workspace and its
    grouped-reduction queue"""
    sid = stream.cuda_stream
    for d in (_WS, ReduceQueue._queues):
        for key in [k for k in d if k[1] == sid]:
            del d[key]


# ---------------------------------------------------------------------------------------------- grouped split-K reductions
class ReduceQueue:
    """Split-K products whose reduction is deferred (valor_gemm_deferred) wait here, each with its own piece of a per-stream group
    workspace, until `flush` sums them in ONE launch per 8 (valor_gemm_reduce_group) and runs their `done` callbacks (the gradient-write
    reports the data-parallel reducer waits for: a parameter is reported only once its final write is enqueued). One queue per stream.
    Flushed when it holds 8 products, when the workspace is full, and at the end of the backward pass that filled it."""
    # products per launch: VALOR_GROUP_REDUCE = 0 (off: one reduction behind every GEMM) | 1 .. 8 (default 8, the kernel's table size)
    GROUP = max(1, min(8, int(os.environ.get("VALOR_GROUP_REDUCE", "8") or 8)))
    BYTES = 1 << 30
    PIECE = _WS_BYTES            # every product is offered what valor_gemm gets: the same slice counts, bit-identical sums
    enabled = os.environ.get("VALOR_GROUP_REDUCE", "8") != "0"
    # VALOR_GROUP_WGRAD=1: an eligible weight gradient (bf16  C += A^T . B  on the 256x256 kernel whose own split would leave at most 48
    # K-tiles per workgroup: the AST / decoder layers' wgrads) is not launched when gemm() is called. It waits here, with references to
    # its operands, and the products of a layer run as ONE launch at flush (valor_gemm_group: a common slice plan, two slices instead of
    # 7 .. 28), followed by the grouped reduction. Default on (profiles/wgrad_group_ab.json, wgrad_group_step_ab.txt); 0: every product
    # is launched when it is issued, exactly as before.
    group_wgrad = os.environ.get("VALOR_GROUP_WGRAD", "1") != "0"
    GROUP_WS = 72 << 20          # partial tiles of one grouped launch: at most 256 work items x 256 KiB, plus the row-sum partials
    _queues = {}
    _armed = False               # an end-of-backward flush is scheduled
    _nqueued = 0                 # queued (not yet launched) products over all streams: guard_write's fast path

    def __init__(self, device, stream):
        import ctypes
        self.stream = stream
        self.ws = torch.empty(self.BYTES, dtype=torch.uint8, device=device)
        self.blobs = (ctypes.c_char * (GEMM_PENDING_BYTES * self.GROUP))()
        self.nd, self.off, self.done, self.dtype = 0, 0, [], None       # nd: products launched, their reduction deferred
        self.targets = set()       # output / row-sum buffers of the pending products (see gemm(): no two of them may be the same)
        # products waiting for their grouped launch: their descriptions, the tensors they will read and write (kept alive until the
        # launch is enqueued) and the storages of their operands (guard_write: nobody may overwrite those before the launch)
        self.gblobs = (ctypes.c_char * (GEMM_PENDING_BYTES * self.GROUP))()
        self.gws = torch.empty(self.GROUP_WS, dtype=torch.uint8, device=device) if self.group_wgrad else None
        self.gn, self.gtiles, self.held, self.operands = 0, 0, [], set()

    @classmethod
    def current(cls, device):
        st = torch.cuda.current_stream(device)
        key = (device.index if device.index is not None else torch.cuda.current_device(), st.cuda_stream)
        q = cls._queues.get(key)
        if q is None:
            q = cls._queues[key] = ReduceQueue(device, st)
        return q

    @property
    def n(self):
        """products that wait for the flush: launched with their reduction deferred, or queued for the grouped launch"""
        return self.nd + self.gn

    @staticmethod
    def tiles(M, N):
        return ((M + 255) // 256) * ((N + 255) // 256)

    def queue(self, dt, M, N, K_, a, lda, b, ldb, out, ldc, alpha, rowsum_out, rowsum_accumulate, done):
        """describe  out += alpha a^T . b  for the next grouped launch; False (nothing queued) if valor_gemm_group does not take it"""
        import ctypes
        if self.gws is None:
            self.gws = torch.empty(self.GROUP_WS, dtype=torch.uint8, device=out.device)
        rc = lib.load().valor_gemm_group_problem(ctypes.addressof(self.gblobs) + GEMM_PENDING_BYTES * self.gn, dt, M, N, K_, _ptr(a), lda, _ptr(b), ldb,
                                                 _ptr(out), ldc, float(alpha), 1, _ptr(rowsum_out), int(rowsum_accumulate))
        if rc == -1:
            return False
        if rc != 0:
            raise lib.ValorHipError(f"valor_gemm_group_problem failed with code {rc}")
        self.dtype = dt
        self.gn += 1
        self.gtiles += self.tiles(M, N)
        ReduceQueue._nqueued += 1
        self.held.append((a, b, out, rowsum_out))
        self.operands |= {a.untyped_storage().data_ptr(), b.untyped_storage().data_ptr()}
        self.done.append(done)
        return True

    def _drop_queued(self):
        ReduceQueue._nqueued -= self.gn
        self.gn, self.gtiles, self.held = 0, 0, []
        self.operands.clear()

    def flush(self):
        import ctypes
        n = self.nd
        if self.gn:
            # the queued products as one launch; their blobs leave it as pending products and join the table of the reduction
            # (queue() and gemm() keep n + gn <= GROUP). The launch goes to the queue's stream, whichever stream is current.
            lib.call("valor_gemm_group", self.stream.cuda_stream, self.dtype, ctypes.cast(self.gblobs, ctypes.c_void_p), self.gn,
                     self.gws.data_ptr(), self.gws.numel())
            ctypes.memmove(ctypes.addressof(self.blobs) + GEMM_PENDING_BYTES * n, self.gblobs, GEMM_PENDING_BYTES * self.gn)
            n += self.gn
        if n:
            lib.call("valor_gemm_reduce_group", self.stream.cuda_stream, self.dtype, ctypes.cast(self.blobs, ctypes.c_void_p), n)
        self._drop_queued()
        done, self.done = self.done, []
        self.nd, self.off = 0, 0
        self.targets.clear()
        for fn in done:
            fn()

    @classmethod
    def flush_all(cls):
        """every queue on its own stream; the CURRENT stream then waits for the others (their sums land in the gradient arena the
        caller is about to read)"""
        cls._armed = False
        cur = torch.cuda.current_stream()
        for q in cls._queues.values():
            if q.n or q.done:
                q.flush()
                if q.stream != cur:
                    cur.wait_stream(q.stream)

    @classmethod
    def discard_stale(cls):
        """top of a forward pass: whatever is still queued (or armed) belongs to a backward pass that never finished -- an exception
        between a deferred product and the end-of-backward flush. Its partial tiles must not be summed into the NEXT step's gradients,
        and a stale `_armed` would keep the next backward from scheduling its flush."""
        stale = cls._armed or any(q.n or q.done for q in cls._queues.values())
        if stale:
            for q in cls._queues.values():
                q.nd, q.off, q.done = 0, 0, []
                q.targets.clear()
                q._drop_queued()          # products that never ran: nothing of them reaches the next step's gradients
            cls._armed = False
        return stale

    @classmethod
    def batch(cls):
        """`with ReduceQueue.batch():` outside a backward pass (tests, tools): deferred / queued products issued inside wait, as they
        would for the end of a backward pass, and are flushed at exit"""
        import contextlib

        @contextlib.contextmanager
        def held():
            prev, cls._armed = cls._armed, True
            try:
                yield
            finally:
                cls._armed = prev
                if not prev:
                    cls.flush_all()
        return held()

    @classmethod
    def _arm(cls):
        if cls._armed:
            return
        try:
            from torch.autograd.variable import Variable
            Variable._execution_engine.queue_callback(cls.flush_all)
            cls._armed = True
        except RuntimeError:          # not inside a backward pass (a direct call from a test): nothing will flush later -- do it now
            cls.flush_all()


def guard_write(*tensors):
    """A kernel is about to WRITE into these caller-supplied buffers (an `out=` / `C +=` target, a static buffer, an in-place update).
    A weight gradient queued for a grouped launch reads its operands later than it was issued: if one of them lives in a storage that
    is written now, its queue is flushed first -- the queued product sees the operand's value at the time it was issued. Freshly
    allocated outputs need no check (the queue holds references: the allocator cannot hand out an operand's memory)."""
    if not ReduceQueue._nqueued:
        return
    st = None
    for t in tensors:
        if t is None:
            continue
        sp = t.untyped_storage().data_ptr()
        for q in ReduceQueue._queues.values():
            if q.gn and sp in q.operands:
                q.flush()
                st = st or torch.cuda.current_stream(t.device)
                if q.stream != st:
                    st.wait_stream(q.stream)


def _rowmajor(t):
    assert t.dim() == 2 and t.stride(1) == 1, "need a 2-D tensor with unit inner stride"
    return t.stride(0)


def gemm(a, b, *, trans_a=False, trans_b=False, bias=None, act=ACT_NONE, want_preact=False,
         dact_aux=None, alpha=1.0, out=None, accumulate=False, out_dtype=None, splitk=True, rowsum_out=None, rowsum_accumulate=False,
         defer_done=None, policy=None):
    """C[M,N] = epi(alpha * op(A) . op(B)^T).  A: [M,K] ([K,M] if trans_a); B: [N,K] ([K,N] if trans_b).
    defer_done (a callable): the caller does not need C before the end of the backward pass (a weight gradient accumulated into the
    arena). If the product is split along K its reduction joins the stream's ReduceQueue and `defer_done` runs when the grouped
    reduction has been enqueued; otherwise it runs at once."""
    _check_gpu(a, b, bias, dact_aux, out)
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N, Kb = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    assert K == Kb, f"contraction mismatch {K} vs {Kb}"
    assert a.dtype == b.dtype
    lda, ldb = _rowmajor(a), _rowmajor(b)
    odt = out_dtype or a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=a.device)
    else:
        guard_write(out)
    assert out.shape == (M, N) and out.dtype == odt
    ldc = _rowmajor(out)
    out_f32 = 1 if (odt == torch.float32 and a.dtype != torch.float32) else 0
    preact = None
    if want_preact:
        preact = torch.empty((M, N), dtype=odt, device=a.device)
        assert _rowmajor(preact) == ldc
    ldaux = _rowmajor(dact_aux) if dact_aux is not None else 0
    if defer_done is not None and splitk and ReduceQueue.enabled and not want_preact and policy is None:
        import ctypes
        q = ReduceQueue.current(a.device)
        dt = dt_of(a)
        # one grouped reduction adds all its products to their outputs from different workgroups of ONE launch: two pending products
        # with the same C (or the same row-sum buffer) would race on a non-atomic read-modify-write (a weight used by two Linears of a
        # shallow stack: the shared-BERT text encoder / decoder, the tied word embedding). Such a product closes the group first.
        tg = {t.data_ptr() for t in (out, rowsum_out) if t is not None}
        if q.n >= q.GROUP or q.off + q.PIECE > q.BYTES or (q.n and q.dtype != dt) or (q.targets & tg):
            q.flush()
        # a grouped launch can only be split while its tiles fill at most half a round of the 256 workgroup slots (valor_gemm_group): a
        # product that would push the queued ones past that closes their group -- at the bench shapes exactly a layer (126 / 108 tiles)
        if q.gn and q.gtiles + q.tiles(M, N) > 128:
            q.flush()
        # the product joins the layer's grouped launch instead of running now: the short-slice wgrads only (the ViT / cross-K|V ones run
        # 225 K-tiles per workgroup alone and keep their launches), with nothing in the epilogue but alpha and C +=
        if (ReduceQueue.group_wgrad and trans_a and trans_b and accumulate and dt == DT_BF16 and not out_f32 and bias is None
                and act == ACT_NONE and dact_aux is None
                and q.queue(dt, M, N, K, a, lda, b, ldb, out, ldc, alpha, rowsum_out, rowsum_accumulate, defer_done)):
            q.targets |= tg
            ReduceQueue._arm()
            return out
        blob = ctypes.addressof(q.blobs) + GEMM_PENDING_BYTES * q.nd
        lib.call("valor_gemm_deferred", _stream(), dt, int(trans_a), int(trans_b), M, N, K,
                 _ptr(a), lda, _ptr(b), ldb, _ptr(out), ldc, _ptr(bias), act, 0, _ptr(dact_aux), ldaux,
                 float(alpha), int(accumulate), out_f32, q.ws.data_ptr() + q.off, q.PIECE, _ptr(rowsum_out), int(rowsum_accumulate), blob)
        used = ctypes.c_int64(0)
        lib.call("valor_gemm_pending_bytes", blob, ctypes.cast(ctypes.byref(used), ctypes.c_void_p))
        if used.value:
            q.dtype = dt
            q.nd += 1
            q.off += used.value
            q.done.append(defer_done)
            q.targets |= tg
            ReduceQueue._arm()
        else:
            defer_done()
        return out
    ws = workspace(a.device) if splitk else None
    if policy is not None:          # a lib.GemmPolicy: this call only, no process-global knob is touched
        import ctypes
        lib.call("valor_gemm_tuned", ctypes.addressof(policy), _stream(), dt_of(a), int(trans_a), int(trans_b), M, N, K,
                 _ptr(a), lda, _ptr(b), ldb, _ptr(out), ldc, _ptr(bias), act, _ptr(preact), _ptr(dact_aux), ldaux,
                 float(alpha), int(accumulate), out_f32, _ptr(ws), (ws.numel() * 4 if ws is not None else 0),
                 _ptr(rowsum_out), int(rowsum_accumulate))
        if defer_done is not None:
            defer_done()
        return (out, preact) if want_preact else out
    lib.call("valor_gemm", _stream(), dt_of(a), int(trans_a), int(trans_b), M, N, K,
             _ptr(a), lda, _ptr(b), ldb, _ptr(out), ldc, _ptr(bias), act, _ptr(preact), _ptr(dact_aux), ldaux,
             float(alpha), int(accumulate), out_f32, _ptr(ws), (ws.numel() * 4 if ws is not None else 0),
             _ptr(rowsum_out), int(rowsum_accumulate))
    if defer_done is not None:
        defer_done()
    return (out, preact) if want_preact else out


_INFER_POLICY = None


def infer_policy():
    """the valor_gemm_policy of inference-only products (ops.linear / ops.mlp under torch.no_grad, the decoding step of valor_amd/decode.py):
    few-row products on the weight-streaming kernel (GEMM family 5, policy key 11; VALOR_GEMM_SKINNY=0 turns it off). The training step does
    not use it: its kernels are the ones its parity evidence was collected on."""
    global _INFER_POLICY
    if _INFER_POLICY is None:
        import os
        _INFER_POLICY = lib.GemmPolicy.make(skinny=int(os.environ.get("VALOR_GEMM_SKINNY", "384")))
    return _INFER_POLICY


def gemm_fuses_rowsum(a, b, trans_a, trans_b):
    """True if valor_gemm can produce the row sums of op(A) (bias gradient) beside this GEMM."""
    if not (trans_a and a.dtype == torch.bfloat16):
        return False
    M, Kd = a.shape[1], a.shape[0]
    N = b.shape[1] if trans_b else b.shape[0]
    return lib.load().valor_gemm_kernel_for(DT_BF16, 1, int(trans_b), M, N, Kd, 0) in (3, 4)


def part_blocks():
    return lib.load().valor_ln_part_blocks()


def bdrln_fwd(x, bias, residual, gamma, beta, eps, *, p_drop=0.0, seed=0, offset=0, write_z=True, inplace_z=False,
              want_y=True, row_scale=None, rows_per_scale=0):
    """z = dropout(x + bias)/(1-p) [* row_scale[row // rows_per_scale]] + residual ; y = LN(z).  Returns (z, y, mean, rstd)."""
    _check_gpu(x, bias, residual, gamma, beta)
    cols = x.shape[-1]
    rows = x.numel() // cols
    assert x.is_contiguous() and (residual is None or residual.is_contiguous())
    z = None
    if write_z:
        if inplace_z:
            guard_write(x)
        z = x if inplace_z else torch.empty_like(x)
    y = torch.empty_like(x) if want_y else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if want_y else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if want_y else None
    lib.call("valor_bdrln_fwd", _stream(), dt_of(x), _ptr(x), _ptr(bias), _ptr(residual), _ptr(gamma), _ptr(beta),
             _ptr(z), _ptr(y), _ptr(mean), _ptr(rstd), rows, cols, float(eps), float(p_drop), int(seed), int(offset),
             _ptr(row_scale), int(rows_per_scale), RNG_BASE)
    return z, y, mean, rstd


def bdrln_bwd(dy, dz_in, z, mean, rstd, gamma, *, p_drop=0.0, seed=0, offset=0, want_dgamma=True, want_dbeta=True,
              want_dbias=False, separate_dx=False, sinks=(None, None, None), row_scale=None, rows_per_scale=0):
    """Returns (dx, dres, dgamma, dbeta, dbias) ; dx is dres when there is no dropout / row scale.
    sinks = (dgamma, dbeta, dbias) tensors to ACCUMULATE the parameter gradients into (the result slot is None then)."""
    ref = dy if dy is not None else dz_in
    _check_gpu(dy, dz_in, z, gamma)
    cols = ref.shape[-1]
    rows = ref.numel() // cols
    nb = part_blocks()
    ws = workspace(ref.device)
    need = 3 * nb * cols
    assert ws.numel() >= need
    pg = ws[0:nb * cols] if (want_dgamma and dy is not None) else None
    pb = ws[nb * cols:2 * nb * cols] if (want_dbeta and dy is not None) else None
    px = ws[2 * nb * cols:3 * nb * cols] if want_dbias else None
    dres = torch.empty_like(ref)
    dx = torch.empty_like(ref) if (p_drop > 0.0 or separate_dx or row_scale is not None) else dres
    lib.call("valor_bdrln_bwd", _stream(), dt_of(ref), _ptr(dy), _ptr(dz_in), _ptr(z), _ptr(mean), _ptr(rstd),
             _ptr(gamma), _ptr(dx), _ptr(dres), _ptr(pg), _ptr(pb), _ptr(px), rows, cols, float(p_drop), int(seed),
             int(offset), _ptr(row_scale), int(rows_per_scale), RNG_BASE)
    outs, args = [], []
    for part, sink in zip((pg, pb, px), sinks):
        if part is None:
            outs.append(None); args += [0, 0, 0]
        elif sink is not None:
            outs.append(None); args += [_ptr(part), _ptr(sink), 1]
        else:
            o = torch.empty(cols, dtype=ref.dtype, device=ref.device)
            outs.append(o); args += [_ptr(part), _ptr(o), 0]
    if any(a for a in args[0::3]):
        lib.call("valor_colsum_finalize3", _stream(), dt_of(ref), *args, nb, cols)
    return dx, dres, outs[0], outs[1], outs[2]


def colsum(x, out=None, accumulate=False):
    """out[cols] (+)= sum over rows of the 2-D tensor x (unit inner stride)."""
    _check_gpu(x, out)
    rows, cols = x.shape
    ld = _rowmajor(x)
    if out is None:
        out = torch.empty(cols, dtype=x.dtype, device=x.device)
        accumulate = False
    else:
        guard_write(out)
    ws = workspace(x.device)
    assert ws.numel() >= part_blocks() * cols
    lib.call("valor_colsum", _stream(), dt_of(x), _ptr(x), rows, cols, ld, _ptr(ws), _ptr(out), 0, int(accumulate))
    return out


def _bsr(t):
    """(batch stride, row stride) of a [B, S, E] view with unit inner stride."""
    assert t.dim() == 3 and t.stride(2) == 1
    return t.stride(0), t.stride(1)


def attn_fwd(q, k, v, n_heads, *, mask=None, kv_range=None, kv_bmod=0, scale=None, p_drop=0.0, seed=0, offset=0, o=None, lse=None):
    """q: [B,Sq,H*64] view, k/v: [Bkv,Skv,H*64] views (unit inner stride). Returns (o [B,Sq,H*64], lse [B,H,Sq])."""
    _check_gpu(q, k, v, mask, kv_range)
    B, Sq, E = q.shape
    Skv = k.shape[1]
    assert E == n_heads * 64, "head_dim is fixed at 64"
    if scale is None:
        scale = 0.125
    guard_write(o, lse)
    if o is None:
        o = torch.empty((B, Sq, E), dtype=q.dtype, device=q.device)
    if lse is None:
        lse = torch.empty((B, n_heads, Sq), dtype=torch.float32, device=q.device)
    assert o.shape == (B, Sq, E) and lse.shape == (B, n_heads, Sq) and lse.is_contiguous()
    qb, qr = _bsr(q); kb, kr = _bsr(k); vb, vr = _bsr(v); ob, orr = _bsr(o)
    mb = mr = 0
    if mask is not None:
        assert mask.dtype == torch.float32 and mask.dim() == 3 and mask.stride(2) == 1
        mb, mr = (mask.stride(0) if mask.shape[0] > 1 else 0), mask.stride(1)
    if kv_range is not None:
        assert kv_range.dtype == torch.int32 and kv_range.shape == (B, 2) and kv_range.is_contiguous()
    lib.call("valor_attn_fwd", _stream(), dt_of(q), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), B, n_heads, Sq, Skv,
             qb, qr, kb, kr, vb, vr, ob, orr, _ptr(mask), mb, mr, _ptr(kv_range), int(kv_bmod), float(scale),
             float(p_drop), int(seed), int(offset), RNG_BASE)
    return o, lse


def attn_decode(q, k, v, n_heads, *, mask=None, key_row=None, scale=0.125, o=None):
    """One decoding step against K|V slots (valor_attn_decode_fwd): q [B, Sq <= 4, H*64], k / v [B, Skv <= 256, H*64] views, additive fp32
    mask [B | 1, Sq, Skv], key_row int32 [B, Skv] (slot j of sequence b is read from batch row key_row[b, j]; None: b). Returns o."""
    _check_gpu(q, k, v, mask, key_row)
    B, Sq, E = q.shape
    Skv = k.shape[1]
    assert E == n_heads * 64, "head_dim is fixed at 64"
    if o is None:
        o = torch.empty((B, Sq, E), dtype=q.dtype, device=q.device)
    qb, qr = _bsr(q); kb, kr = _bsr(k); vb, vr = _bsr(v); ob, orr = _bsr(o)
    mb = mr = 0
    if mask is not None:
        assert mask.dtype == torch.float32 and mask.dim() == 3 and mask.stride(2) == 1
        mb, mr = (mask.stride(0) if mask.shape[0] > 1 else 0), mask.stride(1)
    rb = 0
    if key_row is not None:
        assert key_row.dtype == torch.int32 and key_row.shape == (B, Skv) and key_row.stride(1) == 1
        rb = key_row.stride(0)
    lib.call("valor_attn_decode_fwd", _stream(), dt_of(q), _ptr(q), _ptr(k), _ptr(v), _ptr(o), None, B, n_heads, Sq, Skv,
             qb, qr, kb, kr, vb, vr, ob, orr, _ptr(mask), mb, mr, _ptr(key_row), rb, float(scale))
    return o


def attn_bwd(q, k, v, o, lse, dout, n_heads, *, dq=None, dk=None, dv=None, mask=None, kv_range=None, kv_bmod=0,
             scale=None, p_drop=0.0, seed=0, offset=0, accumulate_kv=False):
    """Returns (dq, dk, dv) shaped like q, k, v (or writes into the given [B,S,H*64] views)."""
    _check_gpu(q, k, v, o, dout, mask, kv_range)
    B, Sq, E = q.shape
    Skv = k.shape[1]
    if scale is None:
        scale = 0.125
    guard_write(dq, dk, dv)
    if dq is None:
        dq = torch.empty((B, Sq, E), dtype=q.dtype, device=q.device)
    if dk is None:
        dk = torch.empty((k.shape[0], Skv, E), dtype=q.dtype, device=q.device)
    if dv is None:
        dv = torch.empty((v.shape[0], Skv, E), dtype=q.dtype, device=q.device)
    delta = torch.empty((B, n_heads, Sq), dtype=torch.float32, device=q.device)
    qb, qr = _bsr(q); kb, kr = _bsr(k); vb, vr = _bsr(v); ob, orr = _bsr(o); gb, gr = _bsr(dout)
    dqb, dqr = _bsr(dq); dkb, dkr = _bsr(dk); dvb, dvr = _bsr(dv)
    mb = mr = 0
    if mask is not None:
        mb, mr = (mask.stride(0) if mask.shape[0] > 1 else 0), mask.stride(1)
    lib.call("valor_attn_bwd", _stream(), dt_of(q), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _ptr(dout), _ptr(dq),
             _ptr(dk), _ptr(dv), _ptr(delta), B, n_heads, Sq, Skv, qb, qr, kb, kr, vb, vr, ob, orr, gb, gr,
             dqb, dqr, dkb, dkr, dvb, dvr, _ptr(mask), mb, mr, _ptr(kv_range), int(kv_bmod), float(scale),
             float(p_drop), int(seed), int(offset), int(accumulate_kv), RNG_BASE)
    return dq, dk, dv


def _xattn_segs(segs, kv_bmod, bwd):
    arr = (lib.XattnSeg * len(segs))()
    for i, sg in enumerate(segs):
        q, o = sg["q"], sg["o"]
        _check_gpu(q, o, sg["lse"], sg.get("kv_range"))
        a = arr[i]
        a.q, a.o, a.lse, a.kv_range = _ptr(q), _ptr(o), _ptr(sg["lse"]), _ptr(sg.get("kv_range"))
        (a.q_bs, a.q_rs), (a.o_bs, a.o_rs) = _bsr(q), _bsr(o)
        if bwd:
            do, dq = sg["dout"], sg["dq"]
            _check_gpu(do, dq)
            a.dout, a.dq = _ptr(do), _ptr(dq)
            (a.do_bs, a.do_rs), (a.dq_bs, a.dq_rs) = _bsr(do), _bsr(dq)
        a.B, a.Sq, a.seed, a.offset = q.shape[0], q.shape[1], int(sg.get("seed", 0)), int(sg.get("offset", 0))
    return arr


def _xattn_domain(segs, k, kv_bmod):
    if k.dtype != torch.bfloat16 or not (1 <= len(segs) <= 2) or k.shape[1] < 64 or kv_bmod <= 0:
        return False
    nsub = sum((sg["q"].shape[0] // kv_bmod) * ((sg["q"].shape[1] + 15) // 16) for sg in segs)
    return not (nsub > 10 or any(sg["q"].shape[0] % kv_bmod for sg in segs) or os.environ.get("VALOR_ATTN_XFUSED", "1") == "0")


def _xattn_call(name, *args):
    """the fused cross-attention entries validate their own domain (strides that are multiples of 8 elements, 16-byte bases, < 2 GiB
    per operand, <= ten 16-row query sub-tiles, the VALOR_ATTN_XFUSED switch as the C side parses it) and answer VALOR_ERR_ARG (-1)
    BEFORE anything is launched when a call falls outside it: that is "not covered" (False -> the caller runs the per-pass kernels),
    not a failure. Every other non-zero code is one."""
    rc = getattr(lib.load(), name)(*args)
    if rc == -1:
        return False
    if rc != 0:
        raise lib.ValorHipError(f"{name} failed with code {rc}")
    return True


def cross_attn_fwd_fused(segs, k, v, n_heads, kv_bmod, *, scale=0.125, p_drop=0.0):
    """Forward of up to two decoder passes that attend to the same K|V in ONE launch (csrc/attention_xu.hip): K, V read once.
    segs: list of dict(q, o [B, T, E] views, lse [B, H, T], kv_range int32 [B, 2] or None, seed, offset); o and lse are written.
    Returns False (nothing launched) outside the fused kernel's domain -- the caller runs attn_fwd per pass."""
    if not _xattn_domain(segs, k, kv_bmod):
        return False
    import ctypes
    guard_write(*[sg["o"] for sg in segs], *[sg["lse"] for sg in segs])
    arr = _xattn_segs(segs, kv_bmod, False)
    kb, kr = _bsr(k); vb, vr = _bsr(v)
    return _xattn_call("valor_cross_attn_fwd_fused", _stream(), DT_BF16, ctypes.cast(arr, ctypes.c_void_p), len(segs), _ptr(k), _ptr(v),
                       n_heads, k.shape[1], int(kv_bmod), kb, kr, vb, vr, float(scale), float(p_drop), RNG_BASE)


def cross_attn_bwd_fused(segs, k, v, dk, dv, n_heads, kv_bmod, *, scale=0.125, p_drop=0.0):
    """Backward of up to two decoder passes that attend to the same K|V in ONE launch (csrc/attention_xu.hip): dK|dV are written once.
    segs: list of dict(q, o, lse, dout, dq [B, T, E] views / lse [B, H, T]; kv_range int32 [B, 2] or None; seed, offset).
    Returns False (nothing launched) when the shape is outside the fused kernel's domain -- the caller runs attn_bwd per pass."""
    if not _xattn_domain(segs, k, kv_bmod):
        return False
    guard_write(dk, dv, *[sg["dq"] for sg in segs])
    arr = _xattn_segs(segs, kv_bmod, True)
    kb, kr = _bsr(k); vb, vr = _bsr(v); dkb, dkr = _bsr(dk); dvb, dvr = _bsr(dv)
    import ctypes
    return _xattn_call("valor_cross_attn_bwd_fused", _stream(), DT_BF16, ctypes.cast(arr, ctypes.c_void_p), len(segs), _ptr(k), _ptr(v), _ptr(dk),
                       _ptr(dv), n_heads, k.shape[1], int(kv_bmod), kb, kr, vb, vr, dkb, dkr, dvb, dvr, float(scale), float(p_drop), RNG_BASE)


# ---------------------------------------------------------------------------------------------- VideoSwin
def win_attn_fwd(qkv, geo, table, n_heads, B):
    """3-D shifted-window attention (head_dim 32) in place on the fused QKV rows [B*rows_per_sample, 3C].
    geo: dict(rowmap int32 [nW*N], rel int32 [N], rel_inv int32 [relc+1], label uint8 [nW*N] | None, nW, N, relc, rows).
    Returns (o, lse)."""
    _check_gpu(qkv, table, geo["rowmap"], geo["rel"], geo["label"])
    C = n_heads * 32
    assert qkv.is_contiguous() and qkv.shape == (B * geo["rows"], 3 * C) and table.is_contiguous() and table.shape[1] == n_heads
    o = torch.empty((qkv.shape[0], C), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B * geo["nW"], n_heads, geo["N"]), dtype=torch.float32, device=qkv.device)
    lib.call("valor_win_attn_fwd", _stream(), dt_of(qkv), _ptr(qkv), _ptr(o), _ptr(lse), _ptr(geo["rowmap"]), _ptr(geo["rel"]),
             _ptr(geo["label"]), _ptr(table), B, geo["nW"], geo["N"], n_heads, table.shape[0], geo["relc"], geo["rows"], 32 ** -0.5)
    return o, lse


def win_attn_bwd(qkv, o, lse, dout, geo, table, n_heads, B, dtable=None):
    """Returns (dqkv, dtable); dtable given -> accumulated into (and None returned in its place)."""
    _check_gpu(qkv, o, dout, table, dtable)
    assert dout.is_contiguous() and dout.shape == o.shape
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    acc = dtable is not None
    if dtable is None:
        dtable = torch.empty_like(table)
    need = lib.load().valor_win_attn_workspace_floats(B, geo["nW"], geo["N"], n_heads)
    if need < 0:
        raise lib.ValorHipError("window attention workspace too large")
    ws = workspace(qkv.device, max(_WS_BYTES, need * 4))
    lib.call("valor_win_attn_bwd", _stream(), dt_of(qkv), _ptr(qkv), _ptr(o), _ptr(lse), _ptr(dout), _ptr(dqkv), _ptr(delta),
             _ptr(geo["rowmap"]), _ptr(geo["rel"]), _ptr(geo["rel_inv"]), _ptr(geo["label"]), _ptr(table), _ptr(dtable), int(acc), _ptr(ws),
             ws.numel() * 4,
             B, geo["nW"], geo["N"], n_heads, table.shape[0], geo["relc"], geo["rows"], 32 ** -0.5)
    return dqkv, (None if acc else dtable)


def patchify3d(video_f32, P, out_dtype):
    """video [B, F, C, H, W] fp32 -> [B*F*(H/P)*(W/P), C*2*P*P] rows of PatchEmbed3D's conv (one zero frame appended)."""
    _check_gpu(video_f32)
    assert video_f32.dtype == torch.float32 and video_f32.is_contiguous()
    B, F, C, H, W = video_f32.shape
    out = torch.empty((B * F * (H // P) * (W // P), C * 2 * P * P), dtype=out_dtype, device=video_f32.device)
    lib.call("valor_patchify3d", _stream(), dt_of(out), _ptr(video_f32), _ptr(out), B, F, C, H, W, P)
    return out


def group_mean_fwd(x2d, X):
    _check_gpu(x2d)
    assert x2d.is_contiguous() and x2d.shape[0] % X == 0
    out = torch.empty((x2d.shape[0] // X, x2d.shape[1]), dtype=x2d.dtype, device=x2d.device)
    lib.call("valor_group_mean_fwd", _stream(), dt_of(x2d), _ptr(x2d), _ptr(out), out.shape[0], X, x2d.shape[1])
    return out


def group_mean_bwd(dout, X):
    _check_gpu(dout)
    dout = dout.contiguous()
    din = torch.empty((dout.shape[0] * X, dout.shape[1]), dtype=dout.dtype, device=dout.device)
    lib.call("valor_group_mean_bwd", _stream(), dt_of(dout), _ptr(dout), _ptr(din), dout.shape[0], X, dout.shape[1])
    return din


def mask_tokens(tokens, k, seed, offset, mask_token, range_start, range_end):
    """BERT token masking with host-drawn per-row counts (valor_mask_tokens): tokens [b, T] int64, k [b] int32 (1 <= k[i] <= the row's
    candidates) -> (tokens_out, labels) [b, T] int64, labels -1 at unselected positions."""
    _check_gpu(tokens, k)
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.dim() == 2
    assert k.dtype == torch.int32 and k.is_contiguous() and k.numel() == tokens.shape[0]
    b, T = tokens.shape
    out, labels = torch.empty_like(tokens), torch.empty_like(tokens)
    lib.call("valor_mask_tokens", _stream(), _ptr(tokens), _ptr(k), b, T, int(seed), int(offset), int(mask_token), int(range_start),
             int(range_end), _ptr(out), _ptr(labels))
    return out, labels


def masked_rows(labels, row_off, n, G=1, Ttot=None, r0=0, idx=None, lab_out=None):
    """gather indices + labels of the positions with labels != -1 (valor_masked_rows), in the order of labels.nonzero() repeated for G
    groups: labels [b, T] int64, row_off [b] int32 = the exclusive cumsum of the per-row counts, n = their total. idx / lab_out: [G*n]
    int64 buffers to write (views into a larger buffer are fine) or None (allocated)."""
    _check_gpu(labels, row_off, idx, lab_out)
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.dim() == 2
    assert row_off.dtype == torch.int32 and row_off.is_contiguous() and row_off.numel() == labels.shape[0]
    b, T = labels.shape
    if idx is None:
        idx = torch.empty(G * n, dtype=torch.int64, device=labels.device)
    if lab_out is None:
        lab_out = torch.empty(G * n, dtype=torch.int64, device=labels.device)
    for t in (idx, lab_out):
        assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == G * n
    lib.call("valor_masked_rows", _stream(), _ptr(labels), _ptr(row_off), b, T, G, T if Ttot is None else int(Ttot), int(r0), int(n),
             _ptr(idx), _ptr(lab_out))
    return idx, lab_out


def _caption_rows(seq, clip_idx):
    """what caption_reward and caption_metrics ask of their id matrix and clip indices -> (R, L, the row pitch)"""
    assert seq.dtype == torch.int64 and seq.dim() == 2 and (seq.stride(1) == 1 or seq.shape[1] == 1)
    R, L = seq.shape
    assert clip_idx.dtype == torch.int32 and clip_idx.is_contiguous() and clip_idx.numel() == R
    return R, L, seq.stride(0) if R > 1 else L


def caption_reward(seq, eos, vocab, clip_idx, tables, reward, cider=None, bleu=None):
    """CIDEr-D + BLEU-4 of every row of seq int64 [R, L] (row pitch = stride(0), L <= 128) against the references of clip clip_idx[r]
    (valor_caption_reward): tables = a lib.RewardTables of device pointers (scst.DeviceCaptionScorer keeps the tensors alive), reward /
    cider / bleu fp64 [R] (the two parts optional). One launch, nothing read back."""
    import ctypes
    _check_gpu(seq, clip_idx, reward, cider, bleu)
    R, L, ld = _caption_rows(seq, clip_idx)
    for t in (reward, cider, bleu):
        assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.numel() == R)
    lib.call("valor_caption_reward", _stream(), _ptr(seq), ld, R, L, int(eos), int(vocab), _ptr(clip_idx), ctypes.addressof(tables),
             _ptr(reward), _ptr(cider), _ptr(bleu))


def caption_metrics(seq, eos, vocab, clip_idx, tables, cider, rouge, bleu, counts, summary):
    """Per-row CIDEr / ROUGE-L / sentence BLEU-1..4 and their integers of seq int64 [R, L] (row pitch = stride(0), L <= 128) against the
    references of clip clip_idx[r], and the corpus values of the R rows (valor_caption_metrics): tables = a lib.CapevalTables of device
    pointers (capeval.DeviceCaptionMetrics keeps the tensors alive), cider / rouge fp64 [R], bleu fp64 [R, 4], counts int32 [R, 10],
    summary int64 [16] (valor_capeval_summary: six fp64 values, ten int64 totals). Two launches, nothing read back."""
    import ctypes
    _check_gpu(seq, clip_idx, cider, rouge, bleu, counts, summary)
    R, L, ld = _caption_rows(seq, clip_idx)
    for t, n in ((cider, R), (rouge, R), (bleu, 4 * R)):
        assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == 10 * R
    assert summary.dtype == torch.int64 and summary.is_contiguous() and summary.numel() == 16
    lib.call("valor_caption_metrics", _stream(), _ptr(seq), ld, R, L, int(eos), int(vocab), _ptr(clip_idx), ctypes.addressof(tables),
             _ptr(cider), _ptr(rouge), _ptr(bleu), _ptr(counts), _ptr(summary))


def sample_tokens(logits, seed, offset, eos, unfinished, tok, sents, logprobs):
    """one step of the sampled decode (valor_sample_tokens): logits fp32 [R, V] (row pitch = stride(0)), unfinished bool [R] (updated in
    place), tok int64 [R] (written: the next input token), sents int64 / logprobs fp32 column views [R] (e.g. sents[:, t]). The caller
    advances `offset` by R * ceil(V / 4) per call."""
    _check_gpu(logits, unfinished, tok, sents, logprobs)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    assert unfinished.dtype == torch.bool and unfinished.is_contiguous() and tok.dtype == torch.int64 and tok.is_contiguous()
    assert sents.dtype == torch.int64 and logprobs.dtype == torch.float32 and sents.dim() == logprobs.dim() == 1
    R, V = logits.shape
    assert unfinished.numel() == tok.numel() == sents.numel() == logprobs.numel() == R
    lib.call("valor_sample_tokens", _stream(), _ptr(logits), logits.stride(0), R, V, int(seed), int(offset), int(eos), _ptr(unfinished), _ptr(tok),
             _ptr(sents), sents.stride(0), _ptr(logprobs), logprobs.stride(0))


def sample_tokens_filtered(logits, seed, offset, eos, unfinished, tok, sents, logprobs, inv_temperature=1.0, top_k=0, top_p=1.0, kept=None,
                           cut=None):
    """sample_tokens with temperature, top-k and nucleus filters (valor_sample_tokens_filtered; the law: include/valor_hip.h): the draw
    comes from softmax over S of y = logits * inv_temperature, S = what top-k (ties at the k-th value kept; 0: off) and then top-p over
    its mass (1: off) leave. kept int32 [R] / cut fp32 [R] (optional) receive |S| and min over S of y. The arguments of sample_tokens
    keep their meaning; with every filter off and no kept / cut this IS sample_tokens."""
    _check_gpu(logits, unfinished, tok, sents, logprobs, kept, cut)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    assert unfinished.dtype == torch.bool and unfinished.is_contiguous() and tok.dtype == torch.int64 and tok.is_contiguous()
    assert sents.dtype == torch.int64 and logprobs.dtype == torch.float32 and sents.dim() == logprobs.dim() == 1
    R, V = logits.shape
    assert unfinished.numel() == tok.numel() == sents.numel() == logprobs.numel() == R
    assert kept is None or (kept.dtype == torch.int32 and kept.is_contiguous() and kept.numel() == R)
    assert cut is None or (cut.dtype == torch.float32 and cut.is_contiguous() and cut.numel() == R)
    lib.call("valor_sample_tokens_filtered", _stream(), _ptr(logits), logits.stride(0), R, V, int(seed), int(offset), int(eos),
             float(inv_temperature), int(top_k), float(top_p), _ptr(unfinished), _ptr(tok), _ptr(sents), sents.stride(0), _ptr(logprobs),
             logprobs.stride(0), None if kept is None else _ptr(kept), None if cut is None else _ptr(cut))


def _constrain_rows(logits, hist, t, active, b, hist_stride_s, hist_stride_k):
    """the checks logits_constrain and trie_constrain share -> (R, V, t, b, hist_stride_s) as the launch takes them"""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    R, V = logits.shape
    t = int(t)
    if hist is not None:
        assert hist.dtype == torch.int64 and hist.stride(-1) == 1 and hist.shape[-1] >= t
        if hist_stride_s is None:
            assert hist.dim() == 2 and hist.shape[0] >= R
            hist_stride_s = hist.stride(0)
    else:
        assert t == 0
    b = R if b is None else int(b)
    if hist is not None and t > 0 and R > 0:            # the furthest token a row reads lies inside the tensor's storage
        last = ((min(R, b) - 1) * int(hist_stride_s) + ((R - 1) // b) * int(hist_stride_k) + t - 1) if b >= 1 else 0
        assert hist.storage_offset() + last < hist.untyped_storage().nbytes() // 8
    assert active is None or (active.dtype in (torch.bool, torch.uint8) and active.is_contiguous() and active.numel() == R)
    return R, V, t, b, int(hist_stride_s or 0)


def logits_constrain(logits, hist, t, eos, penalty=1.0, inv_penalty=1.0, ngram=0, min_len=0, suppress=None, active=None, b=None,
                     hist_stride_s=None, hist_stride_k=0):
    """generation controls of one decoding step, in place (valor_logits_constrain; the law: include/valor_hip.h): logits fp32 [R, V]
    (row pitch = stride(0)); hist int64, unit stride along the tokens (None while t == 0); suppress int32 [n] or None; active bool /
    uint8 [R] or None. Row r reads its t tokens at hist.data_ptr + (r % b) * hist_stride_s + (r / b) * hist_stride_k (elements). The
    default is a row-ordered history [R, >= t]: b = R, hist_stride_s = hist.stride(0). Returns logits."""
    _check_gpu(logits, hist, suppress, active)
    R, V, t, b, hist_stride_s = _constrain_rows(logits, hist, t, active, b, hist_stride_s, hist_stride_k)
    assert suppress is None or (suppress.dtype == torch.int32 and suppress.dim() == 1 and suppress.is_contiguous())
    lib.call("valor_logits_constrain", _stream(), _ptr(logits), logits.stride(0), R, V, None if hist is None else _ptr(hist),
             hist_stride_s, int(hist_stride_k), b, t, int(eos), float(penalty), float(inv_penalty),
             int(ngram), int(min_len), None if suppress is None else _ptr(suppress), 0 if suppress is None else suppress.numel(),
             None if active is None else _ptr(active))
    return logits


def trie_constrain(logits, hist, t, eos, trie, active=None, b=None, hist_stride_s=None, hist_stride_k=0):
    """decoding inside a closed answer set, in place (valor_trie_constrain; the law: include/valor_hip.h): logits fp32 [R, V] (row pitch =
    stride(0)); hist int64 with unit stride along the tokens (None while t == 0), addressed like logits_constrain's; trie = the device
    form of a decode.AnswerSet (child_ptr / child_tok / child_node int32, terminal uint8, root int32 [1 | b]); active bool / uint8 [R]
    or None. Every column that continues no candidate becomes lib.TRIE_FLOOR. Returns logits."""
    _check_gpu(logits, hist, active, trie.child_ptr, trie.child_tok, trie.child_node, trie.terminal, trie.root)
    R, V, t, b, hist_stride_s = _constrain_rows(logits, hist, t, active, b, hist_stride_s, hist_stride_k)
    for a in (trie.child_ptr, trie.child_tok, trie.child_node, trie.root):
        assert a.dtype == torch.int32 and a.dim() == 1 and a.is_contiguous()
    n_nodes, n_edges = trie.child_ptr.numel() - 1, trie.child_tok.numel()
    assert trie.terminal.dtype == torch.uint8 and trie.terminal.is_contiguous() and trie.terminal.numel() == n_nodes
    assert trie.child_node.numel() == n_edges
    lib.call("valor_trie_constrain", _stream(), _ptr(logits), logits.stride(0), R, V, None if hist is None else _ptr(hist),
             hist_stride_s, int(hist_stride_k), b, t, int(eos), _ptr(trie.child_ptr), _ptr(trie.child_tok) if n_edges else None,
             _ptr(trie.child_node) if n_edges else None, _ptr(trie.terminal), _ptr(trie.root), n_nodes, n_edges, trie.root.numel(),
             None if active is None else _ptr(active))
    return logits


def trie_score_level(logits, level_node, b, eos, trie, node_score, final, lse=None, lse_out=None):
    """one trie level (or a chunk of one) of the exact ranking of a closed answer set (valor_trie_score_level; the law:
    include/valor_hip.h): logits fp32 [n_level * b, V] (row pitch = stride(0)), row i * b + s = node level_node[i] (int32 [n_level]),
    sample s; trie = the device form of a decode.AnswerSet; node_score / final fp32 [n_nodes * b], written in place (the children's
    prefix scores, the level's own end-of-answer scores). lse fp32 [rows]: the rows' log-sum-exp (valor_xent_fwd's); None: computed in
    the launch and left in lse_out [rows] when given."""
    _check_gpu(logits, level_node, lse, lse_out, node_score, final, trie.child_ptr, trie.child_tok, trie.child_node, trie.terminal)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows, V = logits.shape
    for a in (level_node, trie.child_ptr, trie.child_tok, trie.child_node):
        assert a.dtype == torch.int32 and a.dim() == 1 and a.is_contiguous()
    n_nodes, n_edges = trie.child_ptr.numel() - 1, trie.child_tok.numel()
    assert trie.terminal.dtype == torch.uint8 and trie.terminal.is_contiguous() and trie.terminal.numel() == n_nodes
    assert trie.child_node.numel() == n_edges and level_node.numel() * int(b) == rows
    for a in (node_score, final):
        assert a.dtype == torch.float32 and a.is_contiguous() and a.numel() == n_nodes * int(b)
    for a in (lse, lse_out):
        assert a is None or (a.dtype == torch.float32 and a.is_contiguous() and a.numel() == rows)
    lib.call("valor_trie_score_level", _stream(), _ptr(logits), logits.stride(0) if rows > 1 else max(logits.stride(0), V), rows, V, int(b),
             _ptr(level_node), None if lse is None else _ptr(lse), None if lse_out is None else _ptr(lse_out), int(eos),
             _ptr(trie.child_ptr), _ptr(trie.child_tok) if n_edges else None, _ptr(trie.child_node) if n_edges else None,
             _ptr(trie.terminal), n_nodes, n_edges, _ptr(node_score), _ptr(final))


def fbank(wave, offsets, slice_idx, tables, melbins, T, mean, std, out=None):
    """log-mel filterbank of the selected slices in the model's layout (valor_fbank): wave = the clips packed back to back, fp32 or int16
    PCM [n]; offsets int64 [B + 1]; slice_idx int32 [B, A] (-1: no audio); tables = preprocess.fbank_tables(...).to_device() (window,
    twiddle, mel_start, mel_ptr, mel_w device tensors + win / shift / P). Returns fp32 [B, A, melbins, T]."""
    _check_gpu(wave, offsets, slice_idx, out, tables.window, tables.twiddle, tables.mel_start, tables.mel_ptr, tables.mel_w)
    assert wave.dtype in (torch.float32, torch.int16) and wave.dim() == 1 and wave.is_contiguous()
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and slice_idx.dtype == torch.int32 and slice_idx.is_contiguous()
    B, A = slice_idx.shape
    assert offsets.numel() == B + 1 and tables.melbins == melbins
    assert tables.window.dtype == tables.twiddle.dtype == torch.float64 and tables.mel_w.dtype == torch.float32
    assert tables.mel_start.dtype == tables.mel_ptr.dtype == torch.int32 and tables.mel_ptr.numel() == melbins + 1
    if out is None:
        out = torch.empty((B, A, melbins, T), dtype=torch.float32, device=slice_idx.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * A * melbins * T
    lib.call("valor_fbank", _stream(), _ptr(wave), int(wave.dtype == torch.int16), wave.numel(), _ptr(offsets), _ptr(slice_idx), B, A,
             tables.win, tables.shift, tables.P, melbins, T, _ptr(tables.window), _ptr(tables.twiddle), _ptr(tables.mel_start),
             _ptr(tables.mel_ptr), _ptr(tables.mel_w), tables.mel_w.numel(), float(mean), float(std), _ptr(out))
    return out


def frames_prepare(pixels, offsets, geom, R, mean, std, antialias=False, out=None):
    """uint8 HWC frames -> normalised fp32 [F, 3, R, R] (valor_frames_prepare): pixels uint8 [n] (the frames packed back to back), offsets
    int64 [F], geom int32 [F, 11] = H, W, top, left, h, w, Hv, Wv, oy, ox, flip per frame; mean / std: 3 host floats each."""
    import ctypes
    _check_gpu(pixels, offsets, geom, out)
    assert pixels.dtype == torch.uint8 and pixels.dim() == 1 and pixels.is_contiguous()
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and geom.dtype == torch.int32 and geom.is_contiguous()
    F = offsets.numel()
    assert geom.shape == (F, 11) and len(mean) == 3 and len(std) == 3
    if out is None:
        out = torch.empty((F, 3, R, R), dtype=torch.float32, device=geom.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == F * 3 * R * R
    lib.call("valor_frames_prepare", _stream(), _ptr(pixels), pixels.numel(), _ptr(offsets), _ptr(geom), F, int(R), int(bool(antialias)),
             (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), _ptr(out))
    return out


def meter_update(table, srcs, rows, keep, take):
    """fold the fp32 device scalars `srcs` into the rows `rows` of the meter table fp32 [R, 8] (valor_meter_update: last / ema / sum / count /
    min / max / nonfinite per row, one launch, nothing is read back). The sources' addresses and the row indices go as kernel arguments."""
    import ctypes
    n = len(srcs)
    if n == 0:
        return table
    _check_gpu(table, *srcs)
    assert table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2 and table.shape[1] == len(lib.METER_FIELDS)
    assert len(rows) == n and all(t.dtype == torch.float32 and t.numel() == 1 for t in srcs)
    lib.call("valor_meter_update", _stream(), _ptr(table), table.shape[0], (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs]),
             (ctypes.c_int32 * n)(*rows), n, float(keep), float(take))
    return table


def stats_scratch_floats(n, ntensors, chunk=1024):
    """fp32 words of scratch valor_arena_grad_stats / valor_arena_update_stats need for an arena of n elements and ntensors tensors"""
    return 4 * (n // chunk) + 2 * ((ntensors + 3) // 4 * 4)


def _check_stats_tables(chunk_group, chunk_tensor, tensor_numel, scratch, tensor_stats, group_stats, n):
    nt, ng = tensor_numel.numel(), group_stats.shape[0]
    assert chunk_group.dtype == torch.int8 and chunk_tensor.dtype == torch.int32 and tensor_numel.dtype == torch.int64
    assert chunk_group.is_contiguous() and chunk_tensor.is_contiguous() and tensor_numel.is_contiguous()
    for t, rows in ((tensor_stats, nt), (group_stats, ng)):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, len(lib.STATS_FIELDS))
    assert scratch.dtype == torch.float32 and scratch.is_contiguous()
    if n > 0:
        chunk = lib.load().valor_adamw_chunk()
        assert n % chunk or (chunk_group.numel() == chunk_tensor.numel() == n // chunk and scratch.numel() >= stats_scratch_floats(n, nt, chunk))
    return nt, ng


def arena_grad_stats(grad, chunk_group, chunk_tensor, tensor_numel, norm_mul, scratch, tensor_stats, group_stats):
    """fields 0-3 (g_sumsq, g_absmax, g_nonfinite, g_norm) of the rows of tensor_stats fp32 [ntensors, 8] and group_stats fp32 [ngroups, 8]
    from the flat gradient arena (valor_arena_grad_stats: three launches, one read of the arena, nothing is read back)"""
    _check_gpu(grad, chunk_group, chunk_tensor, tensor_numel, scratch, tensor_stats, group_stats)
    assert grad.is_contiguous() and grad.dim() == 1
    nt, ng = _check_stats_tables(chunk_group, chunk_tensor, tensor_numel, scratch, tensor_stats, group_stats, grad.numel())
    lib.call("valor_arena_grad_stats", _stream(), dt_of(grad), _ptr(grad), _ptr(chunk_group), _ptr(chunk_tensor), _ptr(tensor_numel), nt,
             grad.numel(), ng, float(norm_mul), _ptr(scratch), _ptr(tensor_stats), _ptr(group_stats))
    return tensor_stats, group_stats


def arena_update_stats(master, exp_avg, exp_avg_sq, chunk_group, chunk_tensor, chunk_bc, tensor_numel, lr, eps, gscale, scratch,
                       tensor_stats, group_stats):
    """fields 4-7 (w_sumsq, u_sumsq, w_norm, u_ratio) from the fp32 master / moment arenas behind the update (valor_arena_update_stats);
    lr: one host float per group, gscale: the device scalar of the clip (non-finite = the step was skipped) or None"""
    import ctypes
    _check_gpu(master, exp_avg, exp_avg_sq, chunk_group, chunk_tensor, chunk_bc, tensor_numel, gscale, scratch, tensor_stats, group_stats)
    n = master.numel()
    for t in (master, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    nt, ng = _check_stats_tables(chunk_group, chunk_tensor, tensor_numel, scratch, tensor_stats, group_stats, n)
    assert chunk_bc.dtype == torch.float32 and chunk_bc.is_contiguous() and chunk_bc.numel() >= 2 * chunk_group.numel() and len(lr) == ng
    lib.call("valor_arena_update_stats", _stream(), _ptr(master), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(chunk_group), _ptr(chunk_tensor),
             _ptr(chunk_bc), _ptr(tensor_numel), nt, n, (ctypes.c_float * ng)(*[float(x) for x in lr]), ng, float(eps), _ptr(gscale),
             _ptr(scratch), _ptr(tensor_stats), _ptr(group_stats))
    return tensor_stats, group_stats
