"""CPU: the host statement of the top-k law (valor_amd/search.py topk_host) against torch's stable sort and against a plain Python sort,
chunk merging, the argument validation of valor_topk_rows / valor_topk_workspace_bytes without a device, and the index file format."""
import ctypes
import math

import pytest
import torch


def _python_topk(rows, k, base=0):
    """(value descending, index ascending), NaN below every number, -inf / -1 padding: a Python sort on explicit keys"""
    vals, idxs = [], []
    for row in rows:
        cand = sorted(((1 if math.isnan(v) else 0, 0.0 if math.isnan(v) else -v, base + c, v) for c, v in enumerate(row)), key=lambda t: t[:3])[:k]
        vals.append([t[3] for t in cand] + [float("-inf")] * (k - len(cand)))
        idxs.append([t[2] for t in cand] + [-1] * (k - len(cand)))
    return torch.tensor(vals, dtype=torch.float32).reshape(len(rows), k), torch.tensor(idxs, dtype=torch.int64).reshape(len(rows), k)


def _same(got, want):
    gv, gi = got
    wv, wi = want
    assert torch.equal(gi, wi)
    assert torch.equal(torch.isnan(gv), torch.isnan(wv)) and torch.equal(torch.nan_to_num(gv, nan=0.0), torch.nan_to_num(wv, nan=0.0))


def _matrix(R, C, seed, ties=True, nan=0.0, ninf=0.0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn((R, C), generator=g)
    if ties:
        s = (s * 4).round() / 4                      # a few dozen distinct values: many ties
    s[torch.rand((R, C), generator=g) < nan] = float("nan")
    s[torch.rand((R, C), generator=g) < ninf] = float("-inf")
    return s


@pytest.mark.parametrize("k", [1, 3, 10, 64])
def test_topk_host_is_the_stable_descending_sort(k):
    from valor_amd.search import topk_host
    s = _matrix(5, 300, 0)
    val, order = torch.sort(s, dim=1, descending=True, stable=True)
    _same(topk_host(s, k), (val[:, :k], order[:, :k]))
    _same(topk_host(s, k, base=2 ** 33), (val[:, :k], order[:, :k] + 2 ** 33))


def test_topk_host_nan_lowest_inf_and_short_rows():
    from valor_amd.search import topk_host
    s = _matrix(4, 40, 1, nan=0.2, ninf=0.1)
    s[0, :] = 0.5                                    # all equal: indices 0 .. k-1
    s[1, 3], s[1, 4] = -0.0, 0.0                     # -0 equals +0: index order decides
    for k in (1, 7, 40, 64):                         # 64 > C: -inf / -1 padding behind the NaNs
        got = topk_host(s, k, base=5)
        _same(got, _python_topk(s.tolist(), k, base=5))
        assert got[1][0, :min(k, 40)].tolist() == list(range(5, 5 + min(k, 40)))
    val, idx = topk_host(s, 64)
    nn = int((~torch.isnan(s[2])).sum())
    assert not torch.isnan(val[2, :nn]).any() and torch.isnan(val[2, nn:40]).all() and (idx[2, 40:] == -1).all()
    assert torch.isinf(val[2, 40:]).all() and (val[2, 40:] < 0).all()
    assert idx[2, nn:40].tolist() == sorted(idx[2, nn:40].tolist())           # NaNs among themselves by index
    _same(topk_host(torch.zeros((3, 0)), 4), (torch.full((3, 4), float("-inf")), torch.full((3, 4), -1, dtype=torch.int64)))


@pytest.mark.parametrize("k", [3, 50])
def test_merging_three_uneven_chunks_equals_one_pass(k):
    from valor_amd.search import topk_host
    s = _matrix(6, 4099, 2, nan=0.05, ninf=0.02)
    want = topk_host(s, k, base=7)
    state = (torch.full((6, k), float("-inf")), torch.full((6, k), -1, dtype=torch.int64))
    c0 = 0
    for n in (100, 1, 3998):
        state = topk_host(s[:, c0:c0 + n], k, base=7 + c0, state=state)
        c0 += n
    _same(state, want)
    _same(topk_host(s[:, :0], k, state=want), want)                           # nothing new: the state comes back


def test_argument_validation_without_gpu():
    """both entry points validate before touching the device"""
    from valor_amd import lib
    so = lib.load()
    n = ctypes.c_int64(-5)
    assert so.valor_topk_workspace_bytes(4, 1000, 10, ctypes.byref(n)) == 0 and n.value >= 4 * 10 * 12 and n.value % 16 == 0
    one = n.value
    assert so.valor_topk_workspace_bytes(1, 1 << 20, 10, ctypes.byref(n)) == 0 and n.value > one            # a long row is split into segments
    assert so.valor_topk_workspace_bytes(0, 1000, 10, ctypes.byref(n)) == 0 and n.value == 0
    assert so.valor_topk_workspace_bytes(4, 1000, 10, None) == -1
    for R, C, k in ((-1, 10, 1), (1, -1, 1), (1, 10, 0), (1, 10, 257)):
        assert so.valor_topk_workspace_bytes(R, C, k, ctypes.byref(n)) == -1
    assert so.valor_topk_workspace_bytes(4, 1000, 10, ctypes.byref(n)) == 0
    buf = (ctypes.c_char * (n.value + 64))()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                                # a 16-byte aligned host address: never dereferenced
    nb = n.value

    def rows(score=p, ld=1000, R=4, C=1000, base=0, k=10, val=p, idx=p, ws=p, ws_bytes=nb):
        return so.valor_topk_rows(None, score, ld, R, C, base, k, 1, val, idx, ws, ws_bytes)

    assert rows(R=0) == 0 and rows(R=0, score=None, ws=None, k=0) == 0        # no rows: no-op
    assert rows(score=None) == -1 and rows(val=None) == -1 and rows(idx=None) == -1 and rows(ws=None) == -1
    assert rows(ld=999) == -1
    assert rows(k=0) == -1 and rows(k=257) == -1
    assert rows(ws_bytes=nb - 1) == -1 and rows(ws=p + 8) == -1               # short, misaligned
    assert rows(score=p + 2) == -1 and rows(idx=p + 4) == -1
    assert rows(base=-1) == -1 and rows(base=2 ** 63 - 1000) == -1 and rows(R=-1) == -1


def _cpu_index(late=False, contra="fine"):
    from valor_amd.search import RetrievalIndex
    g = torch.Generator().manual_seed(3)
    ids = [f"clip{j}" for j in range(9)]
    if contra == "coarse":
        feats = [torch.randn((9, 16), generator=g) for _ in range(2 if late else 1)]
        return RetrievalIndex.from_features(feats, ids=ids, group="tva", contra_type="coarse", late_fusion=late)
    feats = [torch.randn((9, n, 16), generator=g).bfloat16() for n in ((4, 2) if late else (6,))]
    ws = [torch.softmax(torch.randn(f.shape[:2], generator=g), dim=1) for f in feats]
    return RetrievalIndex.from_features(feats, ws, ids, group="tva", late_fusion=late, weights_softmaxed=True)


@pytest.mark.parametrize("late,contra", [(False, "fine"), (True, "fine"), (False, "coarse"), (True, "coarse")])
def test_save_load_round_trip(tmp_path, late, contra):
    from valor_amd.search import RetrievalIndex
    index = _cpu_index(late, contra)
    fp = index.fingerprint()
    assert fp["contra_type"] == contra and fp["late_fusion"] == late and fp["D"] == 16 and fp["group"] == "tva"
    assert fp["tokens"] == ([1, 1] if late else [1]) if contra == "coarse" else fp["tokens"] == ([4, 2] if late else [6])
    index.save(tmp_path / "bank.pt")
    back = RetrievalIndex.load(tmp_path / "bank.pt", "cpu")
    assert back.ids == index.ids and back.fingerprint() == fp and len(back) == 9
    for a, b in zip(index.feats + index.weights, back.feats + back.weights):
        assert (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))
    torch.save({"format": "something else"}, tmp_path / "other.pt")
    with pytest.raises(ValueError):
        RetrievalIndex.load(tmp_path / "other.pt", "cpu")


def test_storage_grows_by_doubling_and_keeps_rows():
    index = _cpu_index()
    first = index.feats[0].clone()
    caps = []
    for r in range(6):
        index.add_features([index.feats[0][:5].clone()], [index.weights[0][:5].clone()], [f"new{r}_{j}" for j in range(5)])
        caps.append(index._feats[0].data.shape[0])
    assert len(index) == 39 and index.ids[9] == "new0_0" and torch.equal(index.feats[0][:9], first)
    assert caps == [18, 36, 36, 36, 36, 72]
    with pytest.raises(ValueError):
        index.add_features([first[:2, :, :8]], [index.weights[0][:2]], ["x", "y"])


def test_refusals():
    from types import SimpleNamespace
    from valor_amd import lib
    from valor_amd.search import RetrievalIndex
    index = _cpu_index()
    q = {"feat_t": torch.zeros((2, 5, 16), dtype=torch.bfloat16)}
    with pytest.raises(lib.ValorHipError):                                    # no CPU fallback
        index.search(None, q, 3)
    with pytest.raises(lib.ValorHipError):
        index.scores(None, q)
    with pytest.raises(ValueError):
        index.search(None, q, 0)
    with pytest.raises(ValueError):
        index.search(None, q, 257)
    with pytest.raises(ValueError):                                           # the model's head differs from the bank's
        index.search(SimpleNamespace(spec=SimpleNamespace(contra_type="coarse", late_fusion=False)), q, 3)
    with pytest.raises(ValueError):
        RetrievalIndex.from_features(torch.zeros((2, 3, 16)), group="va")
    with pytest.raises(lib.ValorHipError):                                    # raw weights are softmaxed by the device kernel
        RetrievalIndex.from_features(torch.zeros((2, 3, 16)), torch.zeros((2, 3)))
