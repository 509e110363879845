"""valor_logits_constrain on the GPU against the host law (decode.constrain_rows_host), bit for bit: every V x R x t of the grid, the
hand-made histories and logit values of tests/test_constrain_cpu.py, every n-gram size x penalty with min_length at t = m - 1 and
t = m, suppress lists with duplicates / ids outside [0, V) / [SEP], rows switched off, a canary in the pad of every row; the history
read through the two beam strides; eager issue == graph replay."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_constrain_cpu import history_rows, host_law, same_bits, settings, special_logits      # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 123.25
INF = float("inf")


def canary_buffer(rows, dev):
    """fp32 host rows [R, V] -> (buffer [R, ld], view [R, V]); ld = V rounded up to 32, plus 32; the pad holds CANARY"""
    R, V = rows.shape
    ld = (V + 31) // 32 * 32 + 32
    buf = torch.full((R, ld), CANARY, dtype=torch.float32, device=dev)
    buf[:, :V] = rows.to(dev)
    return buf, buf[:, :V]


def launch(view, hist_dev, t, pen, n, min_len, sup, eos, act, **kw):
    from valor_amd import kernels as K
    dev = view.device
    sup_dev = sup if torch.is_tensor(sup) else (torch.tensor(sup, dtype=torch.int32, device=dev) if len(sup) else None)
    K.logits_constrain(view, hist_dev if t > 0 else None, t, eos, torch.tensor(pen, dtype=torch.float32).item(),
                       torch.tensor(1.0 / pen, dtype=torch.float32).item(), n, min_len, sup_dev, None if act is None else act.to(dev), **kw)


@pytest.mark.parametrize("V", [5, 37, 1001, 30522])
def test_kernel_equals_the_host_law_bit_for_bit(dev, V):
    g = torch.Generator().manual_seed(V)
    eos = V - 1
    changed = 0
    for R in (1, 3, 64):
        logits = special_logits(R, V, g)
        buf0, _ = canary_buffer(logits, dev)
        for t in (0, 1, 2, 3, 17, 63):
            hist = history_rows(R, V, t, g)
            hist_dev = hist.to(dev)
            for pen, n, min_len, sup, act in settings(V, t, R):
                buf = buf0.clone()
                view = buf[:, :V]
                launch(view, hist_dev, t, pen, n, min_len, sup, eos, act)
                got = buf.cpu()
                want = host_law(logits, hist, t, pen, n, min_len, sup, eos, act)
                assert same_bits(got[:, :V], want), (V, R, t, pen, n, min_len, sup, act is not None)
                assert (got[:, V:] == CANARY).all(), (V, R, t)
                if act is not None:
                    assert same_bits(got[:, :V][~act], logits[~act])
                changed += int((~torch.eq(got[:, :V].view(torch.int32), logits.view(torch.int32))).sum())
    assert changed > 0


def test_history_through_the_beam_strides(dev):
    """beam-major rows r = k * b + s over words kept as [b, beam, max_len]: hist_stride_s = beam * max_len, hist_stride_k = max_len"""
    b, beam, max_len, V, t = 5, 3, 9, 37, 7
    g = torch.Generator().manual_seed(1)
    words = torch.randint(0, 4, (b, beam, max_len), generator=g)
    words[1, 2, :t] = torch.tensor([1, 2, 1, 2, 1, 2, 1])
    words[4, 0, :t] = 3
    logits = special_logits(b * beam, V, g)
    row_hist = words.transpose(0, 1).reshape(b * beam, max_len)                     # row k * b + s reads words[s, k]
    act = torch.ones(b * beam, dtype=torch.bool)
    act[[2, 7]] = False
    for n, pen in ((2, 1.3), (3, 0.5), (1, 1.0)):
        want = host_law(logits, row_hist, t, pen, n, t + 1, (3, 3), V - 1, act)
        buf, view = canary_buffer(logits, dev)
        launch(view, words.to(dev), t, pen, n, t + 1, (3, 3), V - 1, act, b=b, hist_stride_s=beam * max_len, hist_stride_k=max_len)
        assert same_bits(view.cpu(), want) and (buf[:, V:] == CANARY).all()
    # step 0 of a beam search: only the first b rows exist, no history is read
    buf, view = canary_buffer(logits, dev)
    launch(view[:b], None, 0, 1.3, 2, 1, (3,), V - 1, None, b=b, hist_stride_s=beam * max_len, hist_stride_k=max_len)
    got = view.cpu()
    assert same_bits(got[:b], host_law(logits[:b], None, 0, 1.3, 2, 1, (3,), V - 1, None)) and same_bits(got[b:], logits[b:])


def test_eager_issue_equals_graph_replay(dev):
    V, R, t = 1001, 64, 17
    g = torch.Generator().manual_seed(2)
    logits = special_logits(R, V, g)
    hist = history_rows(R, V, t, g)
    hist_dev = hist.to(dev)
    act = torch.ones(R, dtype=torch.bool)
    act[::5] = False
    act_dev = act.to(dev)
    sup = (7, 7, V, V - 1)
    args = (1.3, 3, t + 1, torch.tensor(sup, dtype=torch.int32, device=dev), V - 1)       # (no host-to-device copy inside the capture)
    eager, eview = canary_buffer(logits, dev)
    launch(eview, hist_dev, t, *args, act_dev)
    torch.cuda.synchronize()
    static, sview = canary_buffer(logits, dev)
    fresh = static.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch(sview, hist_dev, t, *args, act_dev)              # warm-up on the capture stream
        static.copy_(fresh)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            launch(sview, hist_dev, t, *args, act_dev)
        static.copy_(fresh)
        graph.replay()
    torch.cuda.synchronize()
    assert same_bits(static.cpu(), eager.cpu())
    assert same_bits(eview.cpu(), host_law(logits, hist, t, 1.3, 3, t + 1, sup, V - 1, act))
