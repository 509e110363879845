"""Training diagnostics: statistics per arena tensor and per optimizer group, computed on the device around the fused update.

The fused path leaves nothing to probe from the host: gradients live in one flat arena, the clip computes one global sum, and the update
kernel clears the gradients in the launch that consumes them. `Diagnostics` asks the optimizer for two more kernels instead --
valor_arena_grad_stats between the clip and the update, valor_arena_update_stats behind the update (include/valor_hip.h has the law) --
which fill a per-tensor and a per-group table on the device. Nothing is read back on the step's path and nothing that is trained is
written: a run with diagnostics is bit-identical to the run without.

  * `scalars()`: 0-dim device views of the group table for LossMeter.update(..., extra=...): they are folded, logged and checkpointed
    like the losses;
  * `snapshot()` / `poll()` / `flush()`: the per-tensor table through pinned slots behind events, LossMeter's pattern; a delivered
    `TensorTable` answers by_tensor(), by_module(depth) and nonfinite_tensors() on the host;
  * `stats_host`: both laws restated in numpy fp64, for checks.
"""
import numpy as np
import torch

from . import kernels
from .lib import STATS_FIELDS

LEVELS = ("grad", "full")
# the ten groups of optim/misc.py:66-77 in model.params.optimizer_group's numbering: 2 * family + (1 if no decay)
FAMILIES = ("basic", "new", "clip_visual", "clip_text", "decoder")
GROUP_NAMES = tuple(f"{fam}_{kind}" for fam in FAMILIES for kind in ("decay", "no_decay"))
_F = {k: i for i, k in enumerate(STATS_FIELDS)}


def _fold(rows, norm_mul):
    """one row from many: sums of the sums of squares and of the count, the maximum of the maxima, norms and ratio recomputed"""
    out = np.zeros(len(STATS_FIELDS), dtype=np.float64)
    if len(rows):
        rows = np.asarray(rows, dtype=np.float64)
        for k in ("g_sumsq", "g_nonfinite", "w_sumsq", "u_sumsq"):
            out[_F[k]] = np.cumsum(rows[:, _F[k]])[-1]          # one addition after the other, in the order of the rows
        out[_F["g_absmax"]] = rows[:, _F["g_absmax"]].max()
    out[_F["g_norm"]] = np.sqrt(out[_F["g_sumsq"]]) * norm_mul
    out[_F["w_norm"]] = np.sqrt(out[_F["w_sumsq"]])
    out[_F["u_ratio"]] = np.sqrt(out[_F["u_sumsq"]]) / (out[_F["w_norm"]] + 1e-12)
    return out


def stats_host(chunk_group, chunk_tensor, tensor_numel, ngroups, grad=None, norm_mul=1.0, master=None, exp_avg=None, exp_avg_sq=None,
               chunk_bc=None, lr=None, eps=1e-6, gscale=1.0, chunk=1024):
    """The laws of valor_arena_grad_stats (when `grad` is given: fields 0-3) and valor_arena_update_stats (when `master`, `exp_avg`,
    `exp_avg_sq`, `chunk_bc` [nchunks, 2] and `lr` [ngroups] are given: fields 4-7) in numpy fp64. Arrays are flat host arrays laid out
    like the arenas. Returns (tensor_stats [ntensors, 8], group_stats [ngroups, 8]) in fp64; the fields of a call that was not asked for
    stay zero. Tensor t covers the tensor_numel[t] elements behind its first chunk -- never the padding; it is active if its first
    chunk's group is >= 0; a group row folds its active tensors in tensor-index order."""
    cg, ct = np.asarray(chunk_group).astype(np.int64), np.asarray(chunk_tensor).astype(np.int64)
    numel = np.asarray(tensor_numel).astype(np.int64)
    nt = len(numel)
    tstats = np.zeros((nt, len(STATS_FIELDS)), dtype=np.float64)
    gid = np.full(nt, -1, dtype=np.int64)
    skipped = not np.isfinite(np.float32(gscale))
    f64 = lambda x, o, n: np.asarray(x[o:o + n], dtype=np.float32).astype(np.float64)
    if chunk_bc is not None:
        chunk_bc = np.asarray(chunk_bc, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    for t in range(nt):
        where = np.nonzero(ct == t)[0]
        if not len(where) or numel[t] <= 0:
            continue
        c0, n = int(where[0]), int(numel[t])
        g = int(cg[c0])
        if g < 0 or g >= ngroups:
            continue
        gid[t] = g
        o = c0 * chunk
        if grad is not None:
            x = f64(grad, o, n)
            fin = np.isfinite(x)
            xf = np.abs(x[fin])
            tstats[t, 0] = (xf * xf).sum()
            tstats[t, 1] = xf.max() if len(xf) else 0.0
            tstats[t, 2] = float((~fin).sum())
        if master is not None:
            w, m, v = f64(master, o, n), f64(exp_avg, o, n), f64(exp_avg_sq, o, n)
            tstats[t, 4] = (w * w).sum()
            if not skipped:
                # the bias corrections are per chunk; a tensor's chunks carry the same pair
                bc = np.repeat(chunk_bc[c0:c0 + (n + chunk - 1) // chunk], chunk, axis=0)[:n]
                u = np.float64(np.float32(lr[g])) * bc[:, 1] / bc[:, 0] * m / (np.sqrt(v) + np.float64(np.float32(eps)))
                tstats[t, 5] = (u * u).sum()
        tstats[t] = _fold([tstats[t]], norm_mul)
    gstats = np.stack([_fold([tstats[t] for t in range(nt) if gid[t] == g], norm_mul) for g in range(ngroups)])
    return tstats, gstats


class TensorTable:
    """a delivered per-tensor table: `step`, `names`, `table` float64 [ntensors, 8] (fields: lib.STATS_FIELDS). Host side only."""

    def __init__(self, step, names, table, norm_mul=1.0):
        self.step, self.names, self.norm_mul = step, list(names), float(norm_mul)
        self.table = np.asarray(table, dtype=np.float64)

    def by_tensor(self):
        """name -> {field: float}"""
        return {n: dict(zip(STATS_FIELDS, (float(x) for x in row))) for n, row in zip(self.names, self.table)}

    def by_module(self, depth=1):
        """tensors folded by the first `depth` components of their dotted names: the sums of squares and the non-finite counts are
        summed, the maxima taken, the norms and the ratio recomputed from the folded sums"""
        buckets = {}
        for n, row in zip(self.names, self.table):
            buckets.setdefault(".".join(n.split(".")[:depth]), []).append(row)
        return {k: dict(zip(STATS_FIELDS, (float(x) for x in _fold(rows, self.norm_mul)))) for k, rows in buckets.items()}

    def nonfinite_tensors(self):
        """the names of the tensors whose gradient held inf / NaN"""
        return [n for n, row in zip(self.names, self.table) if row[_F["g_nonfinite"]] > 0]


class Diagnostics:
    """Diagnostics(optimizer, level='grad' | 'full', every=1): owns the two tables, the tensor_numel table and the scratch of the two
    kernels. Hand it to FusedAdamW.step(diagnostics=...) or, for train_step / accumulation / train_window alike, to
    TrainEngine(diagnostics=...). On the optimizer steps whose index (`step_index`, counted from 0; the engine sets it to
    global_step - 1, so a resumed run keeps the phase) is a multiple of `every`, the optimizer launches valor_arena_grad_stats between
    the clip and the update and, for level='full', valor_arena_update_stats behind the update; on the other steps the tables keep
    their values and `fresh` is False.

    tensor_stats fp32 [ntensors, 8] / group_stats fp32 [10, 8]: fields lib.STATS_FIELDS; tensor_names: the arena's names;
    group_names: GROUP_NAMES. Every rank of a data-parallel run computes the same tables (the arena holds the summed gradient)."""
    SLOTS = 4

    def __init__(self, optimizer, level="grad", every=1):
        if level not in LEVELS:
            raise ValueError(f"Diagnostics: level {level!r}, expected one of {LEVELS}")
        if int(every) < 1:
            raise ValueError("Diagnostics: every must be >= 1")
        self.optimizer, self.level, self.every = optimizer, level, int(every)
        a = optimizer.arena
        self.tensor_names = list(a.offsets)
        self.group_names = list(GROUP_NAMES[:optimizer.N_GROUPS])
        nt = len(self.tensor_names)
        f32 = dict(dtype=torch.float32, device=a.device)
        self.tensor_numel = torch.tensor([n for _, n, _ in a.offsets.values()], dtype=torch.int64).to(a.device)
        self.tensor_stats = torch.zeros((nt, len(STATS_FIELDS)), **f32)
        self.group_stats = torch.zeros((len(self.group_names), len(STATS_FIELDS)), **f32)
        self.scratch = torch.empty(kernels.stats_scratch_floats(a.numel, nt, a.chunk), **f32)
        self.step_index = 0            # the index of the NEXT optimizer step
        self.fresh = False             # the last optimizer step wrote the tables
        self.table_step = None         # index of the step the tables describe
        self.norm_mul = 1.0
        self._slots = [None] * self.SLOTS
        self._free = list(range(self.SLOTS))
        self._pending, self._done = [], []

    # ---- called by FusedAdamW.step
    def due(self):
        """is the optimizer step that begins now a diagnostics step? Advances step_index."""
        self.fresh = self.step_index % self.every == 0
        if self.fresh:
            self.table_step = self.step_index
        self.step_index += 1
        return self.fresh

    def grad_stats(self, chunk_group, norm_mul):
        opt = self.optimizer
        self.norm_mul = float(norm_mul)
        kernels.arena_grad_stats(opt.arena.grad, chunk_group, opt._chunk_tensor, self.tensor_numel, norm_mul, self.scratch,
                                 self.tensor_stats, self.group_stats)

    def update_stats(self, chunk_group, lr):
        opt = self.optimizer
        kernels.arena_update_stats(opt.master, opt.exp_avg, opt.exp_avg_sq, chunk_group, opt._chunk_tensor, opt._chunk_bc, self.tensor_numel,
                                   lr, opt.eps, opt.gscale, self.scratch, self.tensor_stats, self.group_stats)

    # ---- for the meter
    def scalars(self):
        """{key: 0-dim device view of the group table}: grad_norm/<group>, grad_absmax/<group> and, for level='full',
        update_ratio/<group>, weight_norm/<group>. Nothing is read back."""
        keys = [("grad_norm", "g_norm"), ("grad_absmax", "g_absmax")]
        if self.level == "full":
            keys += [("update_ratio", "u_ratio"), ("weight_norm", "w_norm")]
        return {f"{key}/{g}": self.group_stats[i, _F[field]] for key, field in keys for i, g in enumerate(self.group_names)}

    # ---- the per-tensor table to the host
    def _collect(self, entry):
        slot, _, step, norm_mul = entry
        self._free.append(slot)
        return TensorTable(step, self.tensor_names, self._slots[slot].numpy().astype(np.float64), norm_mul)

    def snapshot(self, step=None):
        """enqueue an asynchronous copy of the per-tensor table into one of four pinned slots and an event behind it. Does not wait --
        unless all four slots are in flight, where the oldest is collected first. step: the number the table travels with (default:
        the index of the step it describes)."""
        if not self._free:
            entry = self._pending.pop(0)
            entry[1].synchronize()
            self._done.append(self._collect(entry))
        slot = self._free.pop(0)
        if self._slots[slot] is None:
            self._slots[slot] = torch.empty(tuple(self.tensor_stats.shape), dtype=torch.float32, pin_memory=True)
        self._slots[slot].copy_(self.tensor_stats, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((slot, ev, self.table_step if step is None else step, self.norm_mul))

    def poll(self):
        """the snapshots whose copy has completed, oldest first, as [TensorTable]; never blocks"""
        out, self._done = self._done, []
        while self._pending and self._pending[0][1].query():
            out.append(self._collect(self._pending.pop(0)))
        return out

    def flush(self, step=None):
        """a snapshot of the table as it stands and ONE synchronisation (its event); returns everything outstanding like poll()"""
        self.snapshot(step)
        self._pending[-1][1].synchronize()
        return self.poll()
