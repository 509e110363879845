"""The training driver: what the reference's train.py:40-82, conduct_train's control flow (train_utils.py:277-398) and data/loader.py's
MetaLoader / AccumMetaLoader do around the step -- task-mixing loaders with a restorable position, a device-side loss meter, and
Trainer.fit, which runs TrainEngine.train_step / train_window, evaluate.validate and checkpoint.save_run / resume_run in the reference's
order without giving up what they were built for:

  * the host's lead over the device: no loss is read with .item() (train_utils.py:309 reads every one on every step); the step's
    scalars are folded into running statistics ON the device (LossMeter, valor_meter_update) and come back through asynchronous
    snapshots, so log lines may trail the step by a few steps;
  * decode memory: the decoding sessions a validation round leaves behind are released before training goes on;
  * the loader's position: a checkpoint records which item comes next, also behind a prefetching wrapper, so a resumed run sees the
    uninterrupted run's batches.

Out of scope (the caller's): datasets, file reading, tokenizers, argument parsing, launch scripts; the `adam` / `adamax` choices of
--optim; the submit modes; a window that mixes tasks; train_window at world > 1.

Diagnostics (valor_amd/diagnostics.py, Trainer(diagnostics=...) or the options diag_level / diag_every): per optimizer group the gradient
norm and largest gradient and, at level 'full', the update-to-weight ratio and the weight norm, computed on the device around the fused
update and folded into the meter like the losses; per arena tensor the same through asynchronous snapshots at the logging cadence, and one
log record that names the tensors whose gradient was not finite when a step was skipped.

Weight averaging (valor_amd/ema.py, Trainer(ema=...) or the options ema_decay / ema_warmup / ema_every / ema_eval): validation runs on the
averaged weights, swapped into the arena in place for the round, and the checkpoint carries ckpt/ema_step_N.pt."""
import json
import os
import random
import re

import numpy as np
import torch

from . import checkpoint, decode, evaluate, kernels
from .lib import METER_FIELDS, METER_MAX_SRC
from .optim import FusedAdamW, get_lr_sched

TRAINER_FORMAT = "valor_amd.trainer/1"
ROW_INIT = (0.0, 0.0, 0.0, 0.0, float("inf"), float("-inf"), 0.0, 0.0)
_TRAIN_FILE = re.compile(r"train_step_(\d+)\.rank(\d+)\.pt")


def _opt(opts, key, default=None):
    return opts.get(key, default) if isinstance(opts, dict) else getattr(opts, key, default)


# ------------------------------------------------------------------------------------------------------------------ the loss meter
def meter_host(values, keep, take, row=None):
    """The law of valor_meter_update (include/valor_hip.h) restated in numpy float32 for ONE row: fold `values` in order into `row`
    (default: a fresh row [0, 0, 0, 0, +inf, -inf, 0, 0]) and return the row, float32 [8] = last, ema, sum, count, min, max, nonfinite,
    reserved. Every product and sum is rounded to float32 on its own, as the kernel does (no FMA), so the result is bit-equal."""
    f = np.float32
    r = np.array(ROW_INIT, dtype=f) if row is None else np.array(row, dtype=f)
    keep, take = f(keep), f(take)
    for v in values:
        x = f(v)
        r[0] = x
        if not np.isfinite(x):
            r[6] = f(r[6] + f(1))
            continue
        r[1] = x if r[3] == 0 else f(f(x * take) + f(r[1] * keep))
        r[2] = f(r[2] + x)
        r[3] = f(r[3] + f(1))
        r[4] = np.fmin(r[4], x)
        r[5] = np.fmax(r[5], x)
    return r


class LossMeter:
    """Running statistics of the scalars of the training steps, kept on the device: per key one row of a fp32 table -- last, ema (the
    reference's RunningMeter, utils/logger.py:72-85: value * (1 - smooth) + ema * smooth, the first value as it is), sum, count, min, max
    and the number of non-finite values. update() is one kernel launch and reads nothing back; snapshot() / poll() bring the table to
    the host asynchronously.

    Two deliberate differences from the reference:
      * the reference skips only NaN (logger.py:84), so one inf sticks in its average for the rest of the run; here every non-finite
        value is counted in `nonfinite` and left out of ema / sum / count / min / max;
      * the reference re-creates its meters on every step (train_utils.py:331-334 tests `name`, but the keys are `loss_{name}/{k}`), so
        what it logs is the last value; this meter keeps `last` AND the smoothed value.
    count and nonfinite are fp32 counters: exact up to 2^24 updates of a key."""
    SLOTS = 4
    FORMAT = "valor_amd.meter/1"

    def __init__(self, device, smooth=0.99, rows=64):
        self.device = torch.device(device)
        self.keep, self.take = float(np.float32(smooth)), float(np.float32(1.0 - smooth))       # (float)(1 - 0.99), as RunningMeter
        self.names, self.rows = [], {}
        self.table = self._fresh(rows)
        self._slots = [None] * self.SLOTS         # pinned host copies of the table, allocated at first use
        self._free = list(range(self.SLOTS))
        self._pending = []                        # (slot, event, step, number of rows, host scalars), oldest first
        self._done = []                           # snapshots that were collected early (a slot had to be recycled)
        self._held = None                         # the sources of the last launch

    def _fresh(self, rows):
        t = torch.zeros((rows, len(METER_FIELDS)), dtype=torch.float32, device=self.device)       # fills, no host -> device copy
        t[:, 4].fill_(float("inf"))
        t[:, 5].fill_(float("-inf"))
        return t

    def _row(self, key):
        r = self.rows.get(key)
        if r is None:
            r = self.rows[key] = len(self.names)
            self.names.append(key)
            if r >= self.table.shape[0]:
                grown = self._fresh(2 * self.table.shape[0])
                grown[:self.table.shape[0]].copy_(self.table)
                self.table = grown
        return r

    def update(self, name, loss_dict, extra=None):
        """fold one (micro-)step's scalars in: loss_dict's values under the reference's keys `loss_{name}/{k}` (train_utils.py:334),
        `extra`'s under their own keys (grad_norm, gscale). Values are 0-dim device tensors. A key gets its row at first sight."""
        keys = [f"loss_{name}/{k}" for k in loss_dict] + list(extra or ())
        vals = list(loss_dict.values()) + list((extra or {}).values())
        srcs = []
        for t in vals:
            t = t.detach()
            srcs.append((t if t.dtype == torch.float32 else t.float()).reshape(()))
        rows = [self._row(k) for k in keys]
        for i in range(0, len(srcs), METER_MAX_SRC):
            kernels.meter_update(self.table, srcs[i:i + METER_MAX_SRC], rows[i:i + METER_MAX_SRC], self.keep, self.take)
        self._held = srcs

    def _collect(self, entry):
        slot, _, step, n, host = entry
        self._free.append(slot)
        vals = self._slots[slot][:n].tolist()
        out = dict(host or {})
        out.update({self.names[i]: dict(zip(METER_FIELDS[:7], vals[i])) for i in range(n)})
        return step, out

    def snapshot(self, step=None, host=None):
        """enqueue an asynchronous copy of the table into one of four pinned slots and an event behind it; `host`: host-known scalars
        (lr_ratio) that travel with the snapshot. Does not wait -- unless all four slots are in flight (the host is then four
        snapshots ahead of the device), where the oldest is collected first."""
        n = len(self.names)
        if not self._free:
            entry = self._pending.pop(0)
            entry[1].synchronize()
            self._done.append(self._collect(entry))
        slot = self._free.pop(0)
        buf = self._slots[slot]
        if buf is None or buf.shape[0] < n:
            buf = self._slots[slot] = torch.empty((max(self.table.shape[0], n), len(METER_FIELDS)), dtype=torch.float32, pin_memory=True)
        if n:
            buf[:n].copy_(self.table[:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((slot, ev, step, n, host))

    def poll(self):
        """the snapshots whose copy has completed, oldest first, as [(step, {key: {field: float}})]; never blocks"""
        out, self._done = self._done, []
        while self._pending and self._pending[0][1].query():
            out.append(self._collect(self._pending.pop(0)))
        return out

    def flush(self, step=None, host=None):
        """a snapshot of the table as it stands and ONE synchronisation (its event); returns everything outstanding like poll()"""
        self.snapshot(step, host)
        self._pending[-1][1].synchronize()
        return self.poll()

    def state_dict(self):
        """the table and the row names (one synchronisation): a resumed run continues every average to the bit"""
        n = len(self.names)
        return {"format": self.FORMAT, "names": list(self.names), "table": self.table[:n].cpu(), "keep": self.keep, "take": self.take}

    def load_state_dict(self, sd):
        if sd.get("format") != self.FORMAT:
            raise ValueError(f"LossMeter.load_state_dict: format {sd.get('format')!r}, expected {self.FORMAT!r}")
        self.names = [str(k) for k in sd["names"]]
        self.rows = {k: i for i, k in enumerate(self.names)}
        n = len(self.names)
        self.table = self._fresh(max(self.table.shape[0], n))
        if n:
            self.table[:n].copy_(sd["table"].to(torch.float32))
        self.keep, self.take = float(sd["keep"]), float(sd["take"])


# ------------------------------------------------------------------------------------------------------------------ the loaders
def _sampler_epoch(loader, epoch):
    s = getattr(loader, "sampler", None)
    if s is not None and hasattr(s, "set_epoch"):
        s.set_epoch(epoch)


class _MixLoader:
    """what MetaLoader and AccumMetaLoader share: named loaders with sampling ratios, an endless (name, batch) stream, the epoch
    roll-over of data/loader.py:56-63 / :114-121 (epoch += 1, sampler.set_epoch(epoch) where the loader has one, a fresh iterator) and
    the position.

    Position: state_dict(consumed=n) returns what load_state_dict needs so that the NEXT yielded item is item n (items count from 0), for
    any n within the last HISTORY yields -- a prefetching wrapper has pulled one item more than the trainer has consumed. The state
    holds the generator's state, step, epoch, the task being kept, and per loader its epoch and the batches consumed in it;
    load_state_dict restores them: set_epoch, then loader.skip(k) if the loader offers it (it returns an iterator positioned behind k
    batches), else k batches are drawn and dropped. The resumed stream is exact only for loaders that are functions of (epoch, index)."""
    HISTORY = 4
    FORMAT = "valor_amd.loader/1"

    def __init__(self, loaders, distributed=False, seed=0):
        if not isinstance(loaders, dict) or not loaders:
            raise ValueError("loaders: a non-empty dict {name: loader or (loader, ratio)}")
        self.name2loader, self.sampling_pools = {}, []
        for n, l in loaders.items():
            l, r = l if isinstance(l, tuple) else (l, 1)
            self.name2loader[n] = l
            self.sampling_pools.extend([n] * int(r))
        self.names = list(self.name2loader)
        self.ndata = len(self.names)
        self.distributed = distributed
        self.rng = random.Random(seed)
        self.step, self.epoch, self.yielded = 0, 0, 0
        self.task = self.sampling_pools[0]
        self._pos = {n: [0, 0] for n in self.names}               # per loader: the epoch it runs in, batches consumed in it
        self.name2iter = {n: iter(l) for n, l in self.name2loader.items()}
        self._history = []

    def _pick(self):
        raise NotImplementedError

    def _mark(self):
        version, words, gauss = self.rng.getstate()
        return {"format": self.FORMAT, "kind": type(self).__name__, "yielded": self.yielded, "step": self.step, "epoch": self.epoch,
                "task": self.task, "rng": [int(version), [int(w) for w in words], gauss],
                "loaders": {n: list(p) for n, p in self._pos.items()}}

    def __iter__(self):
        """this iterator runs indefinitely (and continues where the last one stopped: the position lives in the loader)"""
        while True:
            self._history = self._history[-(self.HISTORY - 1):] + [self._mark()]          # the state in front of item `yielded`
            task = self._pick()
            try:
                batch = next(self.name2iter[task])
            except StopIteration:
                self.epoch += 1
                _sampler_epoch(self.name2loader[task], self.epoch)
                self._pos[task] = [self.epoch, 0]
                self.name2iter[task] = iter(self.name2loader[task])
                batch = next(self.name2iter[task])
            self._pos[task][1] += 1
            self.yielded += 1
            yield task, batch

    def state_dict(self, consumed=None):
        consumed = self.yielded if consumed is None else int(consumed)
        if consumed == self.yielded:
            return self._mark()
        for st in self._history:
            if st["yielded"] == consumed:
                return st
        raise ValueError(f"{type(self).__name__}.state_dict: item {consumed} is outside the history (items "
                         f"{max(self.yielded - self.HISTORY, 0)} .. {self.yielded} can be restored; {self.yielded} were yielded)")

    def load_state_dict(self, sd):
        if sd.get("format") != self.FORMAT or sd.get("kind") != type(self).__name__:
            raise ValueError(f"{type(self).__name__}.load_state_dict: state of {sd.get('kind')!r} / {sd.get('format')!r}")
        if set(sd["loaders"]) != set(self.names):
            raise ValueError(f"load_state_dict: saved loaders {sorted(sd['loaders'])}, this loader has {sorted(self.names)}")
        version, words, gauss = sd["rng"]
        self.rng.setstate((int(version), tuple(int(w) for w in words), gauss))
        self.step, self.epoch, self.yielded, self.task = int(sd["step"]), int(sd["epoch"]), int(sd["yielded"]), str(sd["task"])
        self._history = []
        for n, (epoch, k) in sd["loaders"].items():
            loader = self.name2loader[n]
            _sampler_epoch(loader, int(epoch))
            if hasattr(loader, "skip"):
                it = loader.skip(int(k))
            else:
                it = iter(loader)
                for _ in range(int(k)):
                    next(it)
            self._pos[n] = [int(epoch), int(k)]
            self.name2iter[n] = it


class MetaLoader(_MixLoader):
    """data/loader.py:75-124: a task is drawn uniformly from the sampling pool (every name `ratio` times) every `accum_steps` yields and
    kept in between; distributed=True: every rank draws, rank 0's draw is broadcast (any_broadcast).

    One deliberate difference: the draw comes from the loader's own random.Random(seed), not from the global `random` module. The host
    token masker draws from the global module inside the forward pass, and a prefetching wrapper pulls the next item while the
    current one trains: global draws would interleave in an order no checkpoint can restore."""

    def __init__(self, loaders, accum_steps=1, distributed=False, seed=0):
        super().__init__(loaders, distributed, seed)
        self.accum_steps = int(accum_steps)

    def _pick(self):
        if self.step % self.accum_steps == 0:
            task = self.rng.choice(self.sampling_pools)
            if self.distributed:
                box = [task]
                torch.distributed.broadcast_object_list(box, src=0)
                task = box[0]
            self.task = task
        self.step += 1
        return self.task


class AccumMetaLoader(_MixLoader):
    """data/loader.py:22-66: round-robin over the loaders in their order; ndata = len(loaders) items make one optimizer step under
    dataset_mix_type='accum' (train_utils.py:311-317)."""

    def _pick(self):
        self.task = self.names[self.step % self.ndata]
        self.step += 1
        return self.task


# ------------------------------------------------------------------------------------------------------------------ the driver
def get_best_name(eval_name, metric):
    """train_utils.py:258-272"""
    if eval_name.startswith("cap"):
        return "CIDEr"
    if eval_name.startswith("qa"):
        return "accuracy"
    if eval_name.startswith("ret"):
        return "video_ravg" if "video_ravg" in metric else "audio_ravg" if "audio_ravg" in metric else None
    if eval_name.startswith("pt"):
        return None
    raise NotImplementedError(eval_name)


def trainer_file(output_dir, step, rank=None):
    """the trainer's own file beside the three of checkpoint.run_files: ckpt/train_step_N.rank{r}.pt"""
    rank = checkpoint._rank() if rank is None else rank
    return os.path.join(output_dir, "ckpt", f"train_step_{step}.rank{rank}.pt")


class JsonlSink:
    """the default log sink: one JSON object per line in output_dir/log/train.jsonl"""

    def __init__(self, output_dir):
        self.path = os.path.join(output_dir, "log", "train.jsonl")
        os.makedirs(os.path.dirname(self.path), exist_ok=True)

    def __call__(self, step, scalars):
        with open(self.path, "a") as fh:
            fh.write(json.dumps(dict(scalars, step=step)) + "\n")


class Trainer:
    """conduct_train (train_utils.py:277-398) around a TrainEngine. The options are read from engine.opts under the reference's names:
    num_train_steps, valid_steps (else num_train_steps // valid_freq - 1, train_utils.py:512; 0 / neither: no validation, no checkpoint),
    dataset_mix_type, save_best, first_eval, zero_shot (it returns behind the first evaluation, train.py:74-79), remove_before_ckpt.

    train_loader yields (name, batch) endlessly (MetaLoader / AccumMetaLoader); task = name.split('--')[0]. 'random' / 'round-robin':
    every item is an optimizer step (gradient_accumulation_steps only keeps the task, as in the reference); 'accum':
    train_step(batch, task, accum_steps=train_loader.ndata). window=M > 1 on an engine built with contra_window=True: M consecutive
    items -- MetaLoader(accum_steps=M) makes them share one task -- are one train_window. Every micro-step's loss_dict goes to the
    meter, at optimizer steps also `grad_norm` and `gscale` (non-finite when the step was skipped: its `nonfinite` count is the number
    of skipped steps). With diagnostics, the steps that wrote the group table add its rows (`grad_norm/<group>`, `grad_absmax/<group>`, at level
    'full' also `update_ratio/<group>`, `weight_norm/<group>`); without, the trainer's files, log lines and launches are what they were.

    After the optimizer step that makes (global_step + 1) % valid_steps == 0 (train_utils.py:368), once per optimizer step (the
    reference repeats it for every micro-step of an accumulation window that stands at such a step): meter.flush(), evaluate.validate,
    decode.release_sessions, the best-metric bookkeeping of train_utils.py:380-391 (>=), checkpoint.save_run(blocking=False), with
    save_best rank 0's ckpt/best_{eval_name}.pt (utils/save.py:51-55), and the trainer's own ckpt/train_step_N.rank{r}.pt: the
    loader's state at the consumed position, the meter's state, the best-metric history. Older trainer files go with
    remove_before_ckpt once the step that replaces them is complete.

    log_fn(step, scalars) is called on rank 0 with what meter.poll() has completed (snapshots are taken every log_every optimizer steps;
    lr_ratio is host-known and rides along); the default sink is JsonlSink(output_dir) when there is an output_dir."""

    def __init__(self, engine, train_loader, val_loaders=None, output_dir=None, annotations=None, log_fn=None, log_every=200,
                 prefetch=True, window=0, meter=None, diagnostics=None, ema=None):
        if not isinstance(engine.optimizer, FusedAdamW):
            raise TypeError("Trainer: the engine's optimizer is not the fused AdamW (the `adam` / `adamax` choices of --optim are out of scope)")
        self.engine, self.train_loader, self.val_loaders = engine, train_loader, val_loaders
        self.output_dir, self.annotations = output_dir, annotations
        self.log_every, self.prefetch, self.window = int(log_every), bool(prefetch), int(window)
        opts = engine.opts
        self.num_train_steps = int(_opt(opts, "num_train_steps", 0) or 0)
        if self.num_train_steps < 1:
            raise ValueError("Trainer: opts.num_train_steps must be >= 1")
        vs = _opt(opts, "valid_steps")
        if vs is None and _opt(opts, "valid_freq"):
            vs = self.num_train_steps // int(_opt(opts, "valid_freq")) - 1
        self.valid_steps = max(int(vs or 0), 0)
        self.mix = _opt(opts, "dataset_mix_type", "random")
        if self.mix not in ("random", "round-robin", "accum"):
            raise NotImplementedError(f"dataset_mix_type={self.mix}")
        if self.window > 1 and (not getattr(engine, "contra_window", False) or self.mix == "accum"):
            raise ValueError("Trainer: window=M needs an engine built with contra_window=True and dataset_mix_type 'random' / 'round-robin'")
        self.save_best = bool(_opt(opts, "save_best", False))
        self.remove_before_ckpt = bool(_opt(opts, "remove_before_ckpt", True))
        self.rank = checkpoint._rank()
        self.device = engine.model.arena.flat.device if meter is None else getattr(meter, "device", None)
        self.meter = LossMeter(self.device) if meter is None else meter
        self.log_fn = log_fn if log_fn is not None else (JsonlSink(output_dir) if output_dir is not None and self.rank == 0 else None)
        self.consumed = 0                      # items of train_loader the engine has seen
        self.metric_logger, self.best_indicator = {}, {}
        self.validations, self.checkpoints = {}, []
        self._handle = None
        # diagnostics: a Diagnostics of the engine's optimizer, or True / a level ('grad', 'full') to build one; None: the options
        # diag_level (and diag_every) build one when present. It is handed to the engine, which passes it to every optimizer step.
        level = _opt(opts, "diag_level") if diagnostics is None or diagnostics is True else diagnostics
        if diagnostics is True and level is None:
            level = "grad"
        if isinstance(level, str):
            from .diagnostics import Diagnostics
            diagnostics = Diagnostics(engine.optimizer, level=level, every=int(_opt(opts, "diag_every", 1) or 1))
        self.diagnostics = diagnostics
        if diagnostics is not None:
            engine.diagnostics = diagnostics
        # ema: a WeightEMA of the engine's optimizer; None: the engine's own (built from the options ema_decay / ema_warmup / ema_every).
        # ema_eval: which weights a validation round sees -- 'ema' (the default), 'live', or 'both': the averaged weights drive the
        # best-metric bookkeeping and the live weights' numbers ride along under `live/<task>`
        if ema is not None:
            engine.ema = ema
        elif getattr(engine, "ema", None) is None:
            from .ema import from_options
            engine.ema = from_options(engine.optimizer, opts)
        self.ema = engine.ema
        self.ema_eval = str(_opt(opts, "ema_eval", "ema"))
        if self.ema_eval not in ("ema", "live", "both"):
            raise ValueError(f"Trainer: ema_eval must be 'ema', 'live' or 'both', got {self.ema_eval!r}")

    # ---- logging
    def _log(self, results):
        if self.rank == 0 and self.log_fn is not None:
            for step, scalars in results:
                self.log_fn(step, scalars)

    def _log_nonfinite(self, tables):
        """one record per delivered per-tensor table that shows non-finite gradients: {"step": n, "nonfinite_tensors": [names]}"""
        for t in tables:
            bad = t.nonfinite_tensors()
            if bad and self.rank == 0 and self.log_fn is not None:
                self.log_fn(t.step, {"nonfinite_tensors": bad})

    def _host_scalars(self):
        return {"lr_ratio": float(get_lr_sched(self.engine.global_step, self.engine.opts))}

    # ---- validation + checkpoint
    def _validate(self, step):
        if not self.val_loaders:
            return {}
        model = self.engine.model
        live_log = None
        if self.ema is None or self.ema_eval == "live":
            eval_log = evaluate.validate(model, self.val_loaders, annotations=self.annotations, output_dir=self.output_dir, global_step=step)
            decode.release_sessions(model)
        else:
            if self.ema_eval == "both":           # the live weights first, without result files: those hold the averaged weights' output
                live_log = evaluate.validate(model, self.val_loaders, annotations=self.annotations, output_dir=None, global_step=step)
                decode.release_sessions(model)
            with self.ema.applied():
                eval_log = evaluate.validate(model, self.val_loaders, annotations=self.annotations, output_dir=self.output_dir, global_step=step)
                decode.release_sessions(model)
        self.validations[step] = eval_log if live_log is None else dict(eval_log, **{"live/" + k: v for k, v in live_log.items()})
        if live_log is not None and self.rank == 0 and self.log_fn is not None:
            self.log_fn(step, {f"live/{task_name}_{eval_name}": metric for task_name, val_log in live_log.items()
                               for eval_name, metric in val_log.items() if isinstance(metric, dict)})
        if self.rank == 0:
            for task_name, val_log in eval_log.items():
                for eval_name, metric in val_log.items():
                    if not isinstance(metric, dict):
                        continue
                    eval_name = task_name + "_" + eval_name
                    hist = self.metric_logger.setdefault(eval_name, {})
                    hist[str(step)] = metric
                    best = get_best_name(eval_name, metric)
                    if best is not None:
                        better = "best_step" not in hist or metric[best] >= hist["best_value"]
                        if better:
                            hist["best_step"], hist["best_value"] = step, metric[best]
                        self.best_indicator[eval_name] = better
        return eval_log

    def _prune(self, keep):
        d = os.path.join(self.output_dir, "ckpt")
        for name in os.listdir(d):
            m = _TRAIN_FILE.fullmatch(name)
            if m and int(m.group(2)) == self.rank and int(m.group(1)) != keep:
                os.remove(os.path.join(d, name))

    def state_dict(self):
        loader = self.train_loader.state_dict(consumed=self.consumed) if hasattr(self.train_loader, "state_dict") else None
        return {"format": TRAINER_FORMAT, "consumed": int(self.consumed), "loader": [] if loader is None else [loader],
                "meter": self.meter.state_dict(), "metric_logger": self.metric_logger, "best_indicator": self.best_indicator}

    def load_state_dict(self, sd):
        if sd.get("format") != TRAINER_FORMAT:
            raise ValueError(f"Trainer.load_state_dict: format {sd.get('format')!r}, expected {TRAINER_FORMAT!r}")
        if sd["loader"]:
            self.train_loader.load_state_dict(sd["loader"][0])
        self.consumed = int(sd["consumed"])
        self.meter.load_state_dict(sd["meter"])
        self.metric_logger, self.best_indicator = dict(sd["metric_logger"]), dict(sd["best_indicator"])

    def _save(self, step):
        if self.output_dir is None:
            return
        os.makedirs(os.path.join(self.output_dir, "ckpt"), exist_ok=True)
        if self._handle is not None:
            self._handle.wait()                                     # the last checkpoint is complete: the trainer files before it may go
            if self.remove_before_ckpt and self.checkpoints:
                self._prune(self.checkpoints[-1])
        checkpoint._write(self.state_dict(), trainer_file(self.output_dir, step, self.rank))
        if self.save_best and self.rank == 0 and any(self.best_indicator.values()):
            # the weights the best metric was measured on: the averaged ones unless validation ran on the live weights
            averaged = self.ema is not None and self.ema_eval != "live"
            sd = checkpoint._host_copy(self.ema.state_dict()["weights"] if averaged else self.engine.model.state_dict())
            for k, best in self.best_indicator.items():
                if best:
                    checkpoint._write(sd, os.path.join(self.output_dir, "ckpt", f"best_{k}.pt"))
        self._handle = checkpoint.save_run(self.engine, self.output_dir, blocking=False)
        self.checkpoints.append(step)
        if self.remove_before_ckpt and self._handle.done():
            self._prune(step)

    def _validate_and_save(self, step):
        self._log(self.meter.flush(step, self._host_scalars()))
        if self.diagnostics is not None:
            self._log_nonfinite(self.diagnostics.poll())
        self._validate(step)
        self._save(step)

    def _resume(self, allow_inexact):
        if self.output_dir is None:
            raise ValueError("fit(resume=True) needs an output_dir")
        step = checkpoint.latest_step(self.output_dir, self.rank)
        path = None if step is None else trainer_file(self.output_dir, step, self.rank)
        if path is not None and not os.path.exists(path) and not allow_inexact:
            raise FileNotFoundError(f"fit(resume=True): {path} is missing -- without it the loader's position and the meter cannot be "
                                    "restored; pass allow_inexact=True to continue with the loader as it stands")
        step = checkpoint.resume_run(self.engine, self.output_dir, step=step, allow_inexact=allow_inexact)
        path = trainer_file(self.output_dir, step, self.rank)
        if os.path.exists(path):
            self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
        return step

    # ---- the loop
    def _items(self):
        dev = self.device
        if self.prefetch and dev is not None and torch.device(dev).type == "cuda":
            from .hoststage import PrefetchLoader
            if not isinstance(self.train_loader, PrefetchLoader):
                return iter(PrefetchLoader(self.train_loader, dev))
        return iter(self.train_loader)

    def fit(self, resume=False, allow_inexact=False):
        """run to global_step >= num_train_steps; returns {'global_step', 'items', 'checkpoints': [steps], 'validations': {step: eval_log},
        'best': the metric history, 'meter': the final {key: {field: float}}}. resume=True: checkpoint.resume_run, then the trainer's
        file of that step; FileNotFoundError when that file is missing, unless allow_inexact=True."""
        engine, meter, diag = self.engine, self.meter, self.diagnostics
        opts = engine.opts
        if resume:
            self._resume(allow_inexact)
        elif _opt(opts, "first_eval", False):
            self._validate(0)
            if _opt(opts, "zero_shot", False):
                return self._summary({})
        opt = engine.optimizer
        it = self._items()
        ndata = getattr(self.train_loader, "ndata", 1)
        while engine.global_step < self.num_train_steps:
            if self.window > 1:
                items = [next(it) for _ in range(self.window)]
                self.consumed += self.window
                name = items[0][0]
                if any(n != name for n, _ in items):
                    raise ValueError(f"Trainer: a window of {self.window} items mixes tasks {[n for n, _ in items]} "
                                     "(MetaLoader(accum_steps=window) keeps one task per window)")
                loss_dict = engine.train_window([b for _, b in items], name.split("--")[0])
                stepped = True
            else:
                name, batch = next(it)
                self.consumed += 1
                task = name.split("--")[0]
                if self.mix == "accum":
                    before = engine.global_step
                    loss_dict = engine.train_step(batch, task, accum_steps=ndata)
                    stepped = engine.global_step != before
                else:
                    loss_dict = engine.train_step(batch, task)
                    stepped = True
            extra = {"grad_norm": opt.total_norm, "gscale": opt.gscale} if stepped else None
            if stepped and diag is not None and diag.fresh:
                extra.update(diag.scalars())                     # the group rows of a step that wrote them (every `diag_every` steps)
            meter.update(name, loss_dict, extra)
            if not stepped:
                continue
            step = engine.global_step
            if self.rank == 0 and self.log_fn is not None:
                if self.log_every > 0 and step % self.log_every == 0:
                    meter.snapshot(step, self._host_scalars())
                    if diag is not None and diag.table_step is not None:
                        diag.snapshot(step)
                self._log(meter.poll())
                if diag is not None:
                    self._log_nonfinite(diag.poll())
            if self.valid_steps and (step + 1) % self.valid_steps == 0:
                self._validate_and_save(step)
        final = meter.flush(engine.global_step, self._host_scalars())
        self._log(final)
        if diag is not None and diag.table_step is not None:
            self._log_nonfinite(diag.flush(engine.global_step))
        if self._handle is not None:
            self._handle.wait()
            if self.remove_before_ckpt and self.checkpoints:
                self._prune(self.checkpoints[-1])
        if hasattr(self.train_loader, "load_state_dict") and hasattr(self.train_loader, "state_dict"):
            # a prefetching wrapper has pulled one item the engine never saw: the loader goes back to the consumed position
            self.train_loader.load_state_dict(self.train_loader.state_dict(consumed=self.consumed))
        return self._summary(final[-1][1] if final else {})

    def _summary(self, scalars):
        return {"global_step": int(self.engine.global_step), "items": int(self.consumed), "checkpoints": list(self.checkpoints),
                "validations": self.validations, "best": self.metric_logger, "meter": scalars}


def fit(engine, train_loader, resume=False, allow_inexact=False, **kw):
    """Trainer(engine, train_loader, **kw).fit(resume, allow_inexact)"""
    return Trainer(engine, train_loader, **kw).fit(resume=resume, allow_inexact=allow_inexact)
