"""The two diagnostics entry points (valor_arena_grad_stats, valor_arena_update_stats) alternating, six times each, on arenas of VALOR-base
size with the base model's tensor sizes and synthetic data: the subject of a kernel trace, which separates the streaming pass from the
two small reductions behind it (the update's 4.5 GB between two gradient passes also keeps the 0.75 GB gradient arena out of the
last-level cache).

    rocprofv3 --kernel-trace --stats -d OUT -o t --output-format csv -- python tools/diagnostics_kernels.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from valor_amd import kernels, synth
from valor_amd.model.params import param_table

dev = torch.device("cuda:0")
shapes = [s for _, s, _ in param_table(synth.base_spec())]
numel = [int(torch.Size(s).numel()) for s in shapes]
nch = [(n + 1023) // 1024 for n in numel]
nchunks = sum(nch)
n = nchunks * 1024
ct = torch.repeat_interleave(torch.arange(len(numel), dtype=torch.int32), torch.tensor(nch)).to(dev)
cg = (ct % 10).to(torch.int8)
tn = torch.tensor(numel, dtype=torch.int64, device=dev)
grad = torch.randn(n, device=dev).bfloat16()
w, m = torch.randn(n, device=dev), torch.randn(n, device=dev)
v = torch.rand(n, device=dev)
bc = torch.ones(2 * nchunks, device=dev)
gs = torch.ones((), device=dev)
scratch = torch.empty(kernels.stats_scratch_floats(n, len(numel)), device=dev)
ts, gr = torch.zeros((len(numel), 8), device=dev), torch.zeros((10, 8), device=dev)
print("tensors", len(numel), "elements", n, "largest", max(numel))
for _ in range(6):
    kernels.arena_grad_stats(grad, cg, ct, tn, 1.0, scratch, ts, gr)
    kernels.arena_update_stats(w, m, v, cg, ct, bc, tn, [1e-4] * 10, 1e-6, gs, scratch, ts, gr)
torch.cuda.synchronize()
print("ok", float(gr[:, 3].sum()))
