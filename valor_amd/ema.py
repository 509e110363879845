"""Exponential moving average of the weights: one more flat fp32 buffer beside the optimizer's masters, updated by one streaming kernel
behind the fused AdamW (valor_ema_update, valor_amd/csrc/ema.hip), swapped into the parameter arena IN PLACE for evaluation, saved and
resumed to the bit with the rest of the run (valor_amd.checkpoint: ckpt/ema_step_N.pt). The reference has no such thing; its finetuning
schedules pick the best checkpoint from noisy validation numbers (train_utils.py:380-391), which is what an averaged copy is for.

The law (include/valor_hip.h), per element in fp32 with every operation rounded on its own:
    k = updates so far ;  d = min(decay, (1 + k) / (10 + k)) with warm-up, else decay ;  ema += (1 - d) * (w - ema)
so a tensor that never moves (frozen, or inactive in every task of a mix) equals its average exactly and for ever, and the whole arena
-- pads included -- can be averaged on every due step without a table of active tensors. The count lives on the device: a step the
optimizer skipped (non-finite gradient norm, known to the device only) neither moves the average nor advances the count.

Not done: averaging the bf16 parameters instead of the masters, several decays at once, an average of the optimizer's moments, checkpoint
averaging / SWA schedules, a sharded average, the averaged weights as the SCST baseline."""
import contextlib
import weakref

import numpy as np
import torch

from . import lib
from .kernels import _ptr, _stream, dt_of

EMA_FORMAT = "valor_amd.ema/1"


def decay_at(decay, warmup, k):
    """d of update number k + 1 as the kernel computes it: np.float32"""
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + int(k)) / np.float32(10 + int(k)))
    return np.float32(d)


def ema_host(ema, w, decay, warmup, k):
    """The law of valor_ema_update restated in plain fp32 tensor operations (for checks; bit-identical to the kernel): the average after
    update number k + 1, a new tensor. ema, w: fp32 tensors (CPU); k: the number of updates applied before this one."""
    assert ema.dtype == torch.float32 and w.dtype == torch.float32
    a = np.float32(1) - decay_at(decay, warmup, k)                 # one rounding
    t = w - ema                                                    # one rounding per element
    return ema + t * float(a)                                      # a product, then a sum: torch does not fuse them


def applied_to(arena):
    """the WeightEMA whose average the arena holds right now (inside its applied()), or None"""
    return getattr(arena, "_ema_applied", None)


def refuse_applied(arena, what):
    if applied_to(arena) is not None:
        raise RuntimeError(f"{what} inside WeightEMA.applied(): the parameter arena holds the averaged weights, not the training weights")


class WeightEMA:
    """WeightEMA(optimizer, decay, warmup=True, every=1): the average of `optimizer`'s fp32 masters (fp32 parity mode: the masters are the
    parameters). State: one fp32 tensor of arena.numel, seeded from the masters, and a device int32 count. `every` is read by the
    engine: the steps with global_step % every == 0 update.

    The average is seeded when it is built and seeded again whenever the masters are rewritten wholesale (weights loaded after the
    optimizer exists, FusedAdamW.init_master_from / load_state_dict) as long as no update has been launched; after the first update such
    a rewrite leaves it alone."""

    def __init__(self, optimizer, decay, warmup=True, every=1):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"WeightEMA: decay must be in [0, 1], got {decay}")
        if int(every) < 1:
            raise ValueError(f"WeightEMA: every must be >= 1, got {every}")
        self.optimizer, self.model, self.arena = optimizer, optimizer.model, optimizer.arena
        self.decay, self.warmup, self.every = decay, bool(warmup), int(every)
        self.ema = optimizer.master.detach().clone()
        self.count = torch.zeros(1, dtype=torch.int32, device=self.ema.device)
        self._started = False
        self._stash = None                   # the training weights while applied(): compute dtype, allocated at first use and kept
        if not hasattr(optimizer, "_emas"):
            optimizer._emas = []
        optimizer._emas.append(weakref.ref(self))

    # ---- the update
    def update(self, gscale=None):
        """one valor_ema_update on the current stream over optimizer.master; gscale: the optimizer's device scalar (non-finite = the step
        was skipped, the average and the count stay) or None. Reads nothing back."""
        self._started = True
        lib.call("valor_ema_update", _stream(), _ptr(self.optimizer.master), _ptr(self.ema), self.ema.numel(), self.decay, int(self.warmup),
                 _ptr(self.count), _ptr(gscale) if gscale is not None else None)

    @property
    def updates(self):
        """the number of updates applied (read from the device: synchronises with the stream; the only member that does)"""
        return int(self.count.item())

    def masters_rewritten(self):
        """the optimizer's masters were rewritten wholesale: an average that has not started follows them"""
        if not self._started:
            self.ema.copy_(self.optimizer.master)

    def restart(self):
        """the average starts over from the current masters with count 0"""
        self.ema.copy_(self.optimizer.master)
        self.count.zero_()
        self._started = False

    # ---- evaluation on the averaged weights
    def _cast_into(self, flat):
        if flat.dtype == torch.float32:
            flat.copy_(self.ema)                                    # fp32 parity mode: the "cast" is a copy
        else:
            lib.call("valor_cast_from_f32", _stream(), dt_of(flat), _ptr(self.ema), _ptr(flat), flat.numel())

    @contextlib.contextmanager
    def applied(self):
        """Inside, the parameter arena holds the averaged weights (cast to the compute dtype), written IN PLACE: no address changes, so
        captured encoder / decoder graphs, decoding sessions and the static K|V pools stay valid and read the other values. On exit --
        also when the body raises -- the training weights are copied back from a stash. The fp32 masters and the moments are never
        touched (fp32 parity mode: the parameters are the masters, and come back with the stash). Nothing in the model or ops is derived
        from parameter VALUES and kept: there is no cache to refresh. Not re-entrant; TrainEngine.train_step /
        train_window and checkpoint.save_run refuse to run inside."""
        a = self.arena
        if applied_to(a) is not None:
            raise RuntimeError("WeightEMA.applied() is not re-entrant: the arena already holds averaged weights")
        with torch.no_grad():
            if self._stash is None:
                self._stash = torch.empty_like(a.flat)
            self._stash.copy_(a.flat)
            a._ema_applied = self
            try:
                self._cast_into(a.flat)
                yield self
            finally:
                a.flat.copy_(self._stash)
                a._ema_applied = None

    # ---- state
    def flat_state(self):
        """the flat tensors state_dict() is cut from (valor_amd.checkpoint's device-side snapshot copies them in stream order)"""
        return {"ema": self.ema, "ema_count": self.count}

    def state_dict(self, flat=None):
        """{'format', 'weights': the averaged weights as a reference-keyed fp32 state dict, cut from the flat buffer exactly as
        VALOR.state_dict(flat=...) cuts the model's (VALOR.load_state_dict(strict=True) reads it), 'count', 'decay', 'warmup', 'every'}.
        flat: copies of flat_state()'s tensors to cut from (referenced, not cloned); None = the live state, cloned (one synchronisation
        for the count)."""
        if flat is None:
            flat = {"ema": self.ema.clone(), "ema_count": self.count.clone()}
        return {"format": EMA_FORMAT, "weights": self.model.state_dict(flat=flat["ema"]), "count": int(flat["ema_count"].reshape(-1)[0]),
                "decay": float(self.decay), "warmup": bool(self.warmup), "every": int(self.every)}

    def load_state_dict(self, sd):
        """the inverse of state_dict(): weights (strict: every parameter of the model must be there), count and settings"""
        if sd.get("format") != EMA_FORMAT:
            raise ValueError(f"WeightEMA.load_state_dict: format {sd.get('format')!r}, expected {EMA_FORMAT!r}")
        weights = sd["weights"]
        slices = self.optimizer._ref_slices()
        missing = [r for r in slices if r not in weights]
        if missing:
            raise RuntimeError(f"WeightEMA.load_state_dict: missing {missing[:5]}")
        host = torch.zeros(self.ema.numel(), dtype=torch.float32)            # the pads of the arena are zero in masters and average alike
        for r, (o, n, _, _) in slices.items():
            host[o:o + n].copy_(weights[r].detach().to(torch.float32).reshape(-1))
        self.ema.copy_(host)
        self.count.fill_(int(sd["count"]))
        self.decay, self.warmup, self.every = float(sd["decay"]), bool(sd["warmup"]), int(sd["every"])
        self._started = True


def from_options(optimizer, opts):
    """the WeightEMA the options ema_decay (0 = off, the default), ema_warmup (True) and ema_every (1) ask for, or None"""
    get = (lambda k, d: opts.get(k, d)) if isinstance(opts, dict) else (lambda k, d: getattr(opts, k, d))
    decay = float(get("ema_decay", 0.0) or 0.0)
    if decay == 0.0:
        return None
    return WeightEMA(optimizer, decay, warmup=bool(get("ema_warmup", True)), every=int(get("ema_every", 1) or 1))
