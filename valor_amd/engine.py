"""One optimisation step of the pretraining loop (train_utils.py::conduct_train inner body, :302-364):
forward -> sum of losses -> backward (+ overlapped gradient all-reduce) -> warmup-linear LR -> global-norm
clip -> fused AdamW. Losses stay on the device (the reference's per-step `.item()` syncs, :309, are gone;
read them when you log)."""
import gc
import random
import sys

import numpy as np
import torch

from . import dist as vdist
from .ema import refuse_applied
from .ops import DropoutState
from .optim import FusedAdamW, get_lr_sched


ENGINE_FORMAT = "valor_amd.engine/1"


def host_rng_state():
    """Python `random` (the host TokenMasker), numpy's global generator (VideoSwin stochastic depth) and torch's CPU generator as lists /
    tensors / plain numbers: what torch.load(weights_only=True) reads back"""
    version, words, gauss = random.getstate()
    name, keys, pos, has_gauss, cached = np.random.get_state()
    return {"python": {"version": int(version), "words": [int(w) for w in words], "has_gauss": int(gauss is not None),
                       "gauss": float(gauss) if gauss is not None else 0.0},
            "numpy": {"name": str(name), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
                      "cached": float(cached)},
            "torch": torch.get_rng_state()}


def set_host_rng_state(st):
    py, npy = st["python"], st["numpy"]
    random.setstate((int(py["version"]), tuple(int(w) for w in py["words"]), float(py["gauss"]) if py["has_gauss"] else None))
    np.random.set_state((npy["name"], npy["keys"].numpy().astype(np.uint32), int(npy["pos"]), int(npy["has_gauss"]), float(npy["cached"])))
    torch.set_rng_state(st["torch"].cpu().to(torch.uint8))


def micro_batch_size(batch):
    """rows of one micro-batch: of its token tensors, else of its pixels / spectrograms"""
    toks = batch.get("txt_tokens") or {}
    for t in list(toks.values()) + [batch.get("video_pixels"), batch.get("audio_spectrograms")]:
        if t is not None:
            return int(t.shape[0])
    raise ValueError("micro-batch without txt_tokens, video_pixels or audio_spectrograms")


def window_bank(passes):
    """The window bank of TrainEngine.train_window: the feature passes' feat_t / feat_v / feat_a (each a list entry with .feat_t, .feat_v,
    .feat_a, .tokens; a modality the task does not use is None in every entry) concatenated along the rows in micro-batch order --
    micro-batch m owns rows [m b, (m + 1) b), as rank m does in the reference's all-gather -- and made leaves that take a gradient; the
    contrastive text tokens likewise (no gradient)."""
    bank = {}
    for key in ("feat_t", "feat_v", "feat_a"):
        parts = [getattr(p, key) for p in passes]
        if any(f is None for f in parts):
            if not all(f is None for f in parts):
                raise ValueError(f"window bank: {key} is missing from some micro-batches only")
            bank[key] = None
            continue
        bank[key] = torch.cat([f.detach() for f in parts], dim=0).requires_grad_(True)
    toks = [p.tokens for p in passes]
    bank["tokens"] = None if any(t is None for t in toks) else torch.cat(toks, dim=0)
    return bank


def bank_slice(t, m, b):
    """rows of micro-batch m (b rows each) of a bank tensor"""
    return t[m * b:(m + 1) * b]


class TrainEngine:
    def __init__(self, model, opts, optimizer=None, manage_gc=True, graphs=None, contra_window=None, diagnostics=None, ema=None):
        # the reference clips unless grad_norm == -1 (train_utils.py:358): 0 would clip every gradient to zero, a negative value flip
        # its sign -- the fused clip treats any max_norm <= 0 as "off", so such values are refused here instead of silently meaning -1
        grad_norm = float(getattr(opts, "grad_norm", 5.0))
        if not (grad_norm == -1.0 or grad_norm > 0.0):
            raise ValueError(f"grad_norm must be -1 (no clipping) or > 0, got {grad_norm}")
        self.model, self.opts = model, opts
        # graphs: replay the encoders as hipGraphs (valor_amd/graphs.py) -- the CLIP ViT or the VideoSwin encoder (stochastic-depth factors
        # as a graph input), the AST encoder and the CLIP text tower; the decoder (data-dependent masked-row counts) and the shared-BERT text
        # pass stay eager. Default ON since round 6 (bit-identical to eager; interleaved A/B on two boxes, profiles/r06_graphs_ab_*.txt: equal
        # mean throughput, a quarter of the run-to-run spread, half the host time per step); VALOR_GRAPHS=0 / opts.graphs=False / graphs=False: eager.
        import os as _os
        if graphs is None:
            # (not with activation checkpointing: those are the configurations that fill HBM, and a captured encoder keeps its saved
            # activations in a private pool beside whatever the eager warm-up steps left in the caching allocator)
            graphs = _os.environ.get("VALOR_GRAPHS", "1") != "0" and bool(getattr(opts, "graphs", True)) and not getattr(model, "checkpointing", False)
        if graphs and model.arena.flat.is_cuda:
            model.enable_graphs()
        # The cyclic garbage collector fires in the middle of a forward pass (thousands of short-lived autograd objects per
        # step) and stalls kernel submission for 20-40 ms while the GPU drains. Collect at step boundaries instead: the
        # young generation every step, everything every 64 steps.
        self.manage_gc = manage_gc
        if manage_gc:
            gc.disable()
        self.optimizer = optimizer or FusedAdamW(model, opts)
        # diagnostics: a valor_amd.diagnostics.Diagnostics of this optimizer (or None; it may be set later): every optimizer step --
        # train_step, the closing micro-step of an accumulation window, train_window -- hands it to FusedAdamW.step
        self.diagnostics = diagnostics
        self.world = torch.distributed.get_world_size() if vdist.is_dist() else 1
        self.reducer = vdist.Reducer(model.arena)
        if self.world > 1:
            model.gather_fn = vdist.packed_allgather_with_grads
            # torch DDP broadcasts rank 0's parameters when it wraps the model (train_utils.py:232); the reducer replaces DDP, so the
            # replicas are made identical here: parameters, and the optimizer's fp32 masters / moments (bf16 mode / resumed state)
            torch.distributed.broadcast(model.arena.flat, 0)
            for t in ((self.optimizer.master,) if self.optimizer.separate_master else ()) + (self.optimizer.exp_avg, self.optimizer.exp_avg_sq):
                torch.distributed.broadcast(t, 0)
        # ema: a valor_amd.ema.WeightEMA of this optimizer, else the options ema_decay (0 = off, the default) / ema_warmup / ema_every build
        # one -- behind the broadcast: every rank averages the same masters, nothing is communicated. The optimizer steps with
        # global_step % ema.every == 0 update it (the engine's counter: a resumed run keeps the phase); without one no launch is added.
        if ema is None:
            from .ema import from_options
            ema = from_options(self.optimizer, opts)
        self.ema = ema
        self.global_step = 0
        # The host needs ~45 ms to issue a step the GPU runs for ~118 ms: unthrottled it runs many steps ahead, and every tensor that
        # crosses streams (held by its record_stream event until the GPU passes it) then exists once per step in flight -- the caching
        # allocator keeps growing by 172 .. 592 MiB segments for as long as the lead grows (hipMalloc stalls inside steps). Two steps
        # of lead keep the GPU fed; the step waits for the end of the step before the previous one.
        self.max_ahead = int(getattr(opts, "max_steps_ahead", 2))
        self._step_events = []
        # per-step host / device timing for whoever asks (bench.py sets `trace = []`): every optimizer step appends
        # {"wait_ms": host time blocked in the `max_ahead` throttle, "host_ms": host time of the whole call, "head" / "tail": timing events
        # recorded on the step's stream in front of its first and behind its last launch}. tail[n].elapsed_time(head[n+1]) is the time the
        # stream sat idle between two steps because the host had not issued the next one yet; head.elapsed_time(tail) is the step's span
        # on the device. None (the default) records nothing.
        self.trace = None
        # Even with the lead bounded, the working set keeps growing for a few steps after the first one (a block that crossed streams
        # is reusable only once the other stream has passed it, so some tensors exist once per step in flight): 2 + 172 + 592 MiB of
        # hipMalloc inside steps 4-6 of a run, each a device-wide stall. After the second optimizer step the engine therefore
        # allocates and frees `alloc_headroom_mb` of device memory once (one large block + a few small-pool segments): the caching
        # allocator keeps the segments and carves the late growth out of them instead of calling hipMalloc in the middle of a step.
        import os
        self.alloc_headroom_mb = int(os.environ.get("VALOR_ALLOC_HEADROOM_MB", getattr(opts, "alloc_headroom_mb", 1536)))
        self._headroom_done = False
        self.grad_norm = grad_norm
        self._task = None
        # contra_window (argument, else opts.contra_window): train_step on a LIST of micro-batches is one window step (train_window) --
        # the contrastive loss over all the window's rows -- instead of an error
        self.contra_window = bool(getattr(opts, "contra_window", False) if contra_window is None else contra_window)
        self.keep_window = False         # debugging / tests: train_window leaves its bank and the training passes' features in last_window
        self.last_window = None
        self._micro = 0
        self._window_open = False        # the last train_step returned without an optimizer step: partial gradient sums are in the arena
        self._saver = None               # valor_amd.checkpoint's non-blocking writer, once save_run(blocking=False) was used
        # VALOR_DP_CHECK=1 (debug): every rank must have seen the same task sequence in an accumulation window -- the closing micro-step's
        # bucket order (dist.Reducer) is only the same on every rank if it did; checked with one small all-reduce per optimizer step
        self._check_window = _os.environ.get("VALOR_DP_CHECK", "0") == "1"
        self._window_tasks = []
        if getattr(opts, "dataset_mix_type", "random") not in ("random", "round-robin", "accum"):
            raise NotImplementedError(f"dataset_mix_type={opts.dataset_mix_type}")

    def train_step(self, batch, task, accum_steps=1):
        """One iteration of conduct_train's loop body (train_utils.py:302-364). accum_steps = n > 1 is dataset_mix_type='accum'
        (:311-317,341: loss / n, one optimizer step every n iterations, gradients of the n micro-steps -- possibly of different
        tasks -- summed): the arena simply keeps accumulating, the data-parallel reduction runs once per window."""
        if isinstance(batch, (list, tuple)):
            if not self.contra_window:
                raise TypeError("train_step got a list of micro-batches: pass contra_window=True (engine argument or option) to run it as "
                                "one window step, or call train_window")
            if accum_steps != 1:
                raise ValueError("train_step: a list of micro-batches is one window step; accum_steps does not apply")
            return self.train_window(batch, task)
        model = self.model
        refuse_applied(model.arena, "TrainEngine.train_step")
        if not model.arena.grads_bound():
            raise RuntimeError("parameter .grad tensors were detached from the gradient arena (p.grad = None / zero_grad(set_to_none=True) "
                               "on the raw parameters?): call model.zero_grad() (it re-binds) before the next step")
        accum = accum_steps > 1
        if task != self._task:
            self.reducer.reset_task(task)
            self._task = task
        tracing, t_in, wait_s, head = self._enter_step()
        model.train()
        DropoutState.check_restored()      # a restored device-mode state that never met its counter (graphs were on when it was saved)
        DropoutState.begin_step()          # device mode (model.enable_graphs): by-value offsets restart, the device counter advances
        micro = self._micro + 1             # committed only once forward + backward went through: an exception in between must not shift the
        last = (not accum) or micro % accum_steps == 0          # accumulation window's boundary for the next call
        if self.world > 1 and self._check_window:
            self._window_tasks.append(task)
        # accumulation window: the micro-steps before the last only accumulate; the LAST one reduces bucket by bucket from its gradient
        # hooks like an ordinary step (a bucket that is complete in the last micro-step holds the sum of the whole window), so the
        # window's reduction overlaps that backward instead of running behind it
        self.reducer.prepare_backward(defer=accum and not last, closing=accum and last)
        loss_dict = model(batch, task=task, compute_loss=True)
        loss = sum(loss_dict.values())
        (loss / accum_steps if accum else loss).backward()
        self._micro = micro
        if last and self.world > 1 and self._check_window:
            self._assert_same_window()
        if tracing and self.world > 1:
            # what of the gradient exchange is NOT hidden behind backward: the stream reaches r0 when its last backward kernel is done and
            # r1 when the last bucket has arrived
            r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            r0.record()
        active = self.reducer.finish_backward(last=last)
        if tracing and self.world > 1:
            r1.record()
        self._window_open = not last
        loss_dict["total_loss"] = loss.detach()
        if not last:
            return loss_dict
        self._optimizer_step(active, (tracing, t_in, wait_s, head), (r0, r1) if tracing and self.world > 1 else None)
        return loss_dict

    def train_window(self, batches, task):
        """ONE optimizer step on a window of M equally sized micro-batches whose contrastive loss is computed over all N = M * b rows:
        what the reference computes at world size M with micro-batch m as rank m (utils/distributed.py:38-93, pretrain.py:278-291 --
        every rank evaluates the loss on the gathered features and back-propagates its own slice, DDP averages the gradients), where
        train_step(accum_steps=M) sums M steps that each see b - 1 negatives.

        1. feature pass: every micro-batch through the encoders and contrastive heads of the task, no autograd, training mode, no token
           masker; the features and contrastive tokens go into a bank of N rows. The pass draws the dropout windows (VideoSwin: the
           stochastic-depth factors) the training pass of the same micro-batch draws again in 3.
        2. the contrastive block (VALOR.contrastive_loss) ONCE on the bank, the bank's features as leaves: its backward leaves
           G = d contra_loss / d bank and the full gradients of the parameters applied to gathered features (fine-weight heads,
           temperature, va_fusion), which every reference rank computes identically -- DDP's mean leaves them as they are.
        3. training pass: every micro-batch through the ordinary forward without a contrastive loss of its own; one backward from
           (caption + mlm losses) / M and G[m b:(m + 1) b] / M at the micro-batch's features. The arena accumulates.
        4. LR schedule, clip, fused AdamW: the tail of train_step.

        Returns the window's contra_loss, the mean over the micro-batches of the other losses, and total_loss. M = 1 is train_step on
        that batch. A task without contrastive groups ('cap%', 'qa%', SCST, a 'pt_' task without 'contra') has no window-wide term:
        ValueError -- use train_step(accum_steps=M). The step is atomic: no accumulation window is open before or after it."""
        from .model.valor import WindowPass
        model = self.model
        refuse_applied(model.arena, "TrainEngine.train_window")
        batches = list(batches)
        if not batches:
            raise ValueError("train_window: no micro-batches")
        if self.world > 1:
            raise NotImplementedError("train_window with world > 1: bank rows from other ranks are not gathered; use train_step, whose "
                                      "contrastive loss already runs on the ranks' gathered features")
        if self._window_open:
            raise RuntimeError("train_window: an accumulation window is open (the last train_step did not reach its optimizer step); "
                               "close it with its remaining micro-steps first")
        contra_task, contra_ratio = model.task_groups(task)[2:]
        if not contra_task:
            raise ValueError(f"train_window: task {task!r} has no contrastive groups, so nothing spans the window; "
                             "use train_step(batch, task, accum_steps=M)")
        sizes = [micro_batch_size(b) for b in batches]
        if len(set(sizes)) != 1:
            raise ValueError(f"train_window: micro-batches of unequal size {sizes} (the reference's ranks are equal too)")
        if not model.arena.grads_bound():
            raise RuntimeError("parameter .grad tensors were detached from the gradient arena (p.grad = None / zero_grad(set_to_none=True) "
                               "on the raw parameters?): call model.zero_grad() (it re-binds) before the next step")
        M, b = len(batches), sizes[0]
        if task != self._task:
            self.reducer.reset_task(task)
            self._task = task
        entered = self._enter_step()
        model.train()
        DropoutState.check_restored()
        try:
            # ---- 1. feature pass
            np_state = np.random.get_state()               # VideoSwin stochastic depth: the training passes draw the same factors again
            passes, windows = self.feature_pass(batches, task)
            bank = window_bank(passes)
            # ---- 2. one contrastive evaluation on the bank (every backward of the window only accumulates: one reduction-free window)
            self.reducer.prepare_backward(defer=True)
            contra_loss = model.contrastive_loss(bank["feat_t"], bank["feat_v"], bank["feat_a"], bank["tokens"], contra_task, contra_ratio)
            contra_loss.backward()
            self.reducer.finish_backward(last=False)
            # ---- 3. training passes
            np.random.set_state(np_state)
            sums, kept = {}, []
            for m, batch in enumerate(batches):
                tail = DropoutState.offset                  # host-mode dropout: behind every window handed out so far
                DropoutState.rewind(windows[m])
                wp = WindowPass(features_only=False, draws_end=passes[m].draws_end, resume=tail if DropoutState.base is None else None)
                self.reducer.prepare_backward(defer=True)
                out = model(batch, task=task, compute_loss=True, window=wp)
                roots, grads = [], []
                if out:
                    local = sum(out.values())
                    roots.append(local / M if M > 1 else local)
                    grads.append(None)
                for key, f in (("feat_t", wp.feat_t), ("feat_v", wp.feat_v), ("feat_a", wp.feat_a)):
                    if f is not None:
                        g = bank_slice(bank[key].grad, m, b)
                        roots.append(f)
                        grads.append(g / M if M > 1 else g)
                torch.autograd.backward(roots, grads)
                active = self.reducer.finish_backward(last=m == M - 1)
                for k, v in out.items():
                    sums[k] = v.detach() if k not in sums else sums[k] + v.detach()
                if self.keep_window:
                    kept.append({k: f.detach().clone() for k, f in (("feat_t", wp.feat_t), ("feat_v", wp.feat_v), ("feat_a", wp.feat_a))
                                 if f is not None})
        except BaseException:
            # nothing of a failed window may reach a later step: its partial gradient sums and the reducer's record of them go
            model.arena.grad.zero_()
            self.reducer.window = None
            raise
        self.last_window = {"bank": bank, "train_feats": kept} if self.keep_window else None
        loss_dict = {"contra_loss": contra_loss.detach()}
        loss_dict.update({k: (v / M if M > 1 else v) for k, v in sums.items()})
        loss_dict["total_loss"] = sum(loss_dict.values())
        self._optimizer_step(active, entered)
        return loss_dict

    def feature_pass(self, batches, task):
        """Step 1 of train_window on its own: every micro-batch through the encoders and contrastive heads of `task` without autograd, in
        training mode, with the kernels of the training path (ops.replayed_pass) and without the token masker -> (one WindowPass per
        micro-batch holding feat_t / feat_v / feat_a / tokens, the dropout window each pass drew from). Each pass opens a dropout step
        of its own (DropoutState.begin_step), exactly as the training pass of a micro-step would."""
        from .model.valor import WindowPass
        from .ops import replayed_pass
        model = self.model
        model.train()
        passes, windows = [], []
        with torch.no_grad(), replayed_pass():
            for batch in batches:
                DropoutState.begin_step()
                windows.append(DropoutState.window())
                wp = WindowPass(features_only=True)
                model(batch, task=task, compute_loss=True, window=wp)
                passes.append(wp)
        return passes, windows

    def _enter_step(self):
        """top of a call that may end in an optimizer step: the `max_ahead` throttle and, when someone asked for a trace, the timing
        event in front of the call's first launch -> (tracing, host time at entry, seconds blocked in the throttle, head event)"""
        tracing = self.trace is not None and self.model.arena.flat.is_cuda
        t_in = head = None
        if tracing:
            import time as _time
            t_in = _time.perf_counter()
        wait_s = 0.0
        if self.max_ahead > 0 and len(self._step_events) >= self.max_ahead:
            if tracing:
                t_w = _time.perf_counter()
                self._step_events.pop(0).synchronize()
                wait_s = _time.perf_counter() - t_w
            else:
                self._step_events.pop(0).synchronize()
        if tracing:
            head = torch.cuda.Event(enable_timing=True)
            head.record()
        return tracing, t_in, wait_s, head

    def _optimizer_step(self, active, entered, reduce_events=None):
        """the tail of an optimizer step (train_utils.py:344-362): warmup-linear LR, global-norm clip + fused AdamW on the parameters that
        received a gradient, the step's end event for the throttle / the trace, allocator head-room, the generation-0 collection"""
        tracing, t_in, wait_s, head = entered
        model, opt = self.model, self.optimizer
        self.global_step += 1
        if getattr(self.opts, "num_train_steps", 0):
            ratio = get_lr_sched(self.global_step, self.opts)                      # train_utils.py:344-347
            for g in opt.param_groups:
                g["lr"] = g["init_lr"] * ratio
        kw = {}
        if self.ema is not None and self.global_step % self.ema.every == 0:
            kw["ema"] = self.ema                                       # all arena tensors, active in this task or not (valor_amd/ema.py)
        if self.diagnostics is None:
            opt.step(active_names=active, max_grad_norm=self.grad_norm, world_size=self.world, **kw)   # clip :358-360, step :362
        else:
            self.diagnostics.step_index = self.global_step - 1         # a resumed run keeps the phase of `every`
            opt.step(active_names=active, max_grad_norm=self.grad_norm, world_size=self.world, diagnostics=self.diagnostics, **kw)
        if self.max_ahead > 0 and model.arena.flat.is_cuda:
            ev = torch.cuda.Event(enable_timing=tracing)
            ev.record()
            self._step_events.append(ev)
            if tracing:
                import time as _time
                self.trace.append({"wait_ms": wait_s * 1e3, "host_ms": (_time.perf_counter() - t_in) * 1e3, "head": head, "tail": ev,
                                   "reduce": reduce_events})
        if not self._headroom_done and self.global_step >= 2:
            self.reserve_headroom()
        if self.manage_gc:
            gc.collect(0 if self.global_step % 64 else 2)

    def _assert_same_window(self):
        import zlib
        h = zlib.crc32("|".join(self._window_tasks).encode()) & 0x7fffffff
        self._window_tasks = []
        dev = self.model.arena.flat.device
        t = torch.tensor([h, -h], dtype=torch.int64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        if int(t[0]) != -int(t[1]):
            raise RuntimeError("data-parallel ranks saw different task sequences inside one accumulation window: the gradient buckets of the "
                               "closing micro-step would be reduced in different orders (valor_amd/dist.py)")

    def reserve_headroom(self, mb=None):
        """grow the caching allocator's pools by `mb` MiB of free segments now (see __init__); returns the bytes reserved. A pure
        optimisation: the request is clamped to a quarter of the device memory that is free right now (a configuration that fills HBM
        -- VALOR-large at 16 frames holds 182-191 GB -- must not be pushed over the edge by head-room it does not need), and an
        out-of-memory answer to any of the allocations skips the reservation instead of ending the step: in data parallel one rank
        dying here while the others continue would hang the next collective."""
        self._headroom_done = True
        mb = self.alloc_headroom_mb if mb is None else mb
        dev = self.model.arena.flat.device
        if mb <= 0 or dev.type != "cuda":
            return 0
        from . import streams
        before = torch.cuda.memory_reserved(dev)
        cs = streams.compute_streams(dev)
        free_mb = torch.cuda.mem_get_info(dev)[0] >> 20
        mb = min(mb, free_mb // (4 * max(len(cs), 1)))
        if mb < 64:
            return 0
        # the caching allocator keeps one free list PER STREAM: the late growth happens on the encoders' side stream as well as on the
        # step's stream (the first version reserved on the current stream only and two 172 MiB segments still appeared)
        for st in cs:
            with torch.cuda.stream(st):
                try:
                    blocks = [torch.empty(mb << 20, dtype=torch.uint8, device=dev)]
                    blocks += [torch.empty(1 << 20, dtype=torch.uint8, device=dev) for _ in range(16)]    # small pool (requests <= 1 MiB): 2 MiB segments
                except torch.cuda.OutOfMemoryError:
                    blocks = None
                    break
                del blocks
        return torch.cuda.memory_reserved(dev) - before

    # ---- exact resume: everything outside model and optimizer that the next step's bits depend on (valor_amd.checkpoint.save_run /
    # resume_run write and read it as engine_step_N.rank{r}.pt beside the reference's model_step_N.pt / optimizer_step_N.pt)
    def state_dict(self):
        """Tensors, ints, floats, strings, lists and dicts only (torch.load(weights_only=True) reads it). Reads the dropout counter back
        from the device (one synchronisation). Not inside an accumulation window: the partial gradient sums are not part of a
        checkpoint (in the reference neither: utils/save.py:38-64 saves model and optimizer)."""
        if self._window_open:
            raise RuntimeError("TrainEngine.state_dict: an accumulation window is open (the last train_step did not reach its optimizer "
                               "step); save after the window's closing micro-step")
        from . import decode
        model = self.model
        sd = {"format": ENGINE_FORMAT, "world_size": int(self.world), "rank": torch.distributed.get_rank() if vdist.is_dist() else 0,
              "global_step": int(self.global_step), "micro": int(self._micro), "task": [] if self._task is None else [str(self._task)],
              "dropout": DropoutState.state(), "token_masker": str(getattr(model, "token_masker", "host")), "host_rng": host_rng_state()}
        masker = getattr(model, "device_masker", None)
        if masker is not None:
            sd["device_masker"] = masker.state()
        sampler = decode.sampler_state(model)
        if sampler is not None:
            sd["sampler"] = sampler
        return sd

    def load_state_dict(self, sd):
        """Restore state_dict(). Order-free: before or after model.enable_graphs() (a device-mode dropout state loaded in host mode waits
        for the counter and is written INTO it -- ops.DropoutState.set_state), before or after the model's and the optimizer's own loads
        (nothing here touches parameters or optimizer state). ValueError when the world size, the dropout mode (it follows graphs on /
        off) or the token-masker mode differ from the saved run's: the draws would differ."""
        from . import decode
        if sd.get("format") != ENGINE_FORMAT:
            raise ValueError(f"TrainEngine.load_state_dict: format {sd.get('format')!r}, expected {ENGINE_FORMAT!r}")
        if int(sd["world_size"]) != self.world:
            raise ValueError(f"TrainEngine.load_state_dict: saved with world size {sd['world_size']}, this run has {self.world} "
                             "(per-rank RNG streams and the batch split would differ)")
        model = self.model
        mode = str(getattr(model, "token_masker", "host"))
        if sd["token_masker"] != mode:
            raise ValueError(f"TrainEngine.load_state_dict: saved with token_masker={sd['token_masker']!r}, the model has {mode!r}")
        if self._window_open:
            raise RuntimeError("TrainEngine.load_state_dict: an accumulation window is open")
        DropoutState.set_state(sd["dropout"])               # refuses a host-mode state in device mode before anything else is changed
        self.global_step, self._micro = int(sd["global_step"]), int(sd.get("micro", 0))
        task = sd["task"][0] if sd["task"] else None
        if task != self._task:
            self.reducer.reset_task(task)
            self._task = task
        if mode == "device":
            model.device_masker.set_state(sd["device_masker"])
        decode.set_sampler_state(model, sd.get("sampler"))
        set_host_rng_state(sd["host_rng"])

    def close(self):
        """release what the engine holds outside the Python heap: the native reducer's communicator / stream / events (dist.Reducer.close);
        waits for a non-blocking checkpoint that is still being written; idempotent, also run when the engine is collected"""
        s = getattr(self, "_saver", None)
        if s is not None:
            s.wait()
        r = getattr(self, "reducer", None)
        if r is not None:
            r.close()

    def __del__(self):
        # not at interpreter shutdown: the process group / HIP runtime may be gone by then and a native crash in the communicator's
        # destructor cannot be caught -- call close() (before dist.destroy_process_group) in a driver that wants the resources back
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass
