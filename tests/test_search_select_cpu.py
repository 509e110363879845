"""CPU: the host statement of valor_topk_rows_select (topk_select_host) against a brute-force loop on tie-heavy matrices, its chunk
folding, the entry's argument refusals, and the bookkeeping RetrievalIndex keeps around the selection on a CPU index (kept, saved and
loaded, never searched): remove / live, compact and its map, update, the group label table, persistence with and without the new keys."""
import ctypes

import pytest
import torch


def _same(got, want):
    assert torch.equal(got[1], want[1]), (got[1], want[1])
    assert torch.equal(torch.isnan(got[0]), torch.isnan(want[0]))
    assert torch.equal(torch.nan_to_num(got[0], nan=0.0), torch.nan_to_num(want[0], nan=0.0))


def _matrix(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((R, C), generator=g) * 8).round() / 8          # ties


def _brute(score, k, base=0, keep=None, group=None):
    """the law, one candidate at a time: eligible candidates in (value descending, index ascending) order, NaN last; the first member
    of a group met stands for it"""
    R, C = score.shape
    val = torch.full((R, k), float("-inf"))
    idx = torch.full((R, k), -1, dtype=torch.int64)
    for r in range(R):
        table = lambda t, i: t[i] if t.dim() == 1 else t[r, i]
        cands = [(score[r, c].item(), base + c) for c in range(C) if keep is None or bool(table(keep, base + c))]
        cands.sort(key=lambda t: (t[0] != t[0], -t[0] if t[0] == t[0] else 0.0, t[1]))
        seen, out = set(), []
        for v, i in cands:
            g = -1 if group is None else int(table(group, i))
            if g >= 0 and g in seen:
                continue
            seen.add(g)
            out.append((v, i))
        for p, (v, i) in enumerate(out[:k]):
            val[r, p], idx[r, p] = v, i
    return val, idx


@pytest.mark.parametrize("C", [1, 7, 64, 257])
def test_host_law_equals_brute_force(C):
    from valor_amd.search import topk_host, topk_select_host
    g = torch.Generator().manual_seed(C)
    s = _matrix(5, C, C)
    s[1, torch.rand(C, generator=g) < 0.2] = float("nan")
    s[2, torch.rand(C, generator=g) < 0.2] = float("-inf")
    N = C + 3                                                          # the tables cover base + C entries
    keep1, keep2 = torch.rand(N, generator=g) < 0.7, torch.rand((5, N), generator=g) < 0.5
    grp1 = torch.randint(-1, 6, (N,), generator=g, dtype=torch.int32)
    grp2 = torch.randint(-1, 3, (5, N), generator=g, dtype=torch.int32)
    for k in (1, 3, 10, 64):
        _same(topk_select_host(s, k), topk_host(s, k))
        _same(topk_select_host(s, k, base=3), topk_host(s, k, base=3))
        for keep in (None, keep1, keep2, torch.zeros(N, dtype=torch.bool)):
            for group in (None, grp1, grp2, torch.zeros(N, dtype=torch.int32)):
                _same(topk_select_host(s, k, base=3, keep=keep, group=group), _brute(s, k, 3, keep, group))


@pytest.mark.parametrize("k", [3, 50])
def test_folding_chunks_equals_one_pass(k):
    """a group's best member in the last chunk replaces the representative, one in the first chunk makes later members vanish"""
    from valor_amd.search import topk_select_host
    C = 1203
    s = _matrix(4, C, 9)
    g = torch.Generator().manual_seed(1)
    keep = torch.rand(C, generator=g) < 0.8
    group = (torch.arange(C) % 37).int()
    group[::11] = -1
    s[0, 1202], s[1, 0] = 100.0, 100.0                                 # group 1202 % 37 = 18 wins late; group 0 wins early
    want = topk_select_host(s, k, keep=keep, group=group)
    assert want[1][0, 0] == 1202 and want[1][1, 0] == 0
    for chunks in ((400, 1, 802), (802, 1, 400)):
        state = (torch.full((4, k), float("-inf")), torch.full((4, k), -1, dtype=torch.int64))
        c0 = 0
        for n in chunks:
            state = topk_select_host(s[:, c0:c0 + n], k, base=c0, state=state, keep=keep, group=group)
            c0 += n
        _same(state, want)
    # an entry of the state that the filter no longer admits drops out
    gone = keep.clone()
    gone[want[1][0, 0]] = False
    again = topk_select_host(s[:, :0], k, state=want, keep=gone, group=group)
    assert int(want[1][0, 0]) not in again[1][0].tolist()


def test_argument_validation_without_gpu():
    """both entries validate before touching the device: valor_topk_rows' grounds, a negative keep_ld / group_ld, a misaligned group"""
    from valor_amd import lib
    so = lib.load()
    n, m = ctypes.c_int64(-5), ctypes.c_int64(-5)
    assert so.valor_topk_select_workspace_bytes(4, 1000, 10, ctypes.byref(n)) == 0 and n.value % 16 == 0
    assert so.valor_topk_workspace_bytes(4, 1000, 10, ctypes.byref(m)) == 0 and n.value >= m.value
    assert so.valor_topk_select_workspace_bytes(0, 1000, 10, ctypes.byref(m)) == 0 and m.value == 0
    assert so.valor_topk_select_workspace_bytes(4, 1000, 10, None) == -1
    for R, C, k in ((-1, 10, 1), (1, -1, 1), (1, 10, 0), (1, 10, 257)):
        assert so.valor_topk_select_workspace_bytes(R, C, k, ctypes.byref(m)) == -1
    buf = (ctypes.c_char * (n.value + 64))()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                                # a 16-byte aligned host address: never dereferenced
    nb = n.value

    def rows(score=p, ld=1000, R=4, C=1000, base=0, k=10, keep=p, keep_ld=0, group=p, group_ld=0, val=p, idx=p, ws=p, ws_bytes=nb):
        return so.valor_topk_rows_select(None, score, ld, R, C, base, k, 1, keep, keep_ld, group, group_ld, val, idx, ws, ws_bytes)

    assert rows(R=0) == 0 and rows(R=0, score=None, ws=None, k=0) == 0        # no rows: no-op
    assert rows(score=None) == -1 and rows(val=None) == -1 and rows(idx=None) == -1 and rows(ws=None) == -1
    assert rows(ld=999) == -1
    assert rows(k=0) == -1 and rows(k=257) == -1
    assert rows(ws_bytes=nb - 1) == -1 and rows(ws=p + 8) == -1               # short, misaligned
    assert rows(score=p + 2) == -1 and rows(idx=p + 4) == -1
    assert rows(base=-1) == -1 and rows(base=2 ** 63 - 1000) == -1 and rows(R=-1) == -1
    assert rows(keep_ld=-1) == -1 and rows(group_ld=-1) == -1 and rows(group=p + 2) == -1
    assert rows(keep=None, keep_ld=-1) == -1 and rows(group=None, group_ld=-5) == -1


# ------------------------------------------------------------------ the index's bookkeeping
def _cpu_index(bank_dtype=None, groups=None, n=9):
    """a fine index on the CPU: bf16 features, or (bank_dtype) codes of the right shapes with an exact store in host memory"""
    from valor_amd.search import RetrievalIndex
    g = torch.Generator().manual_seed(3)
    ids = [f"clip{j}" for j in range(n)]
    feats = torch.randn((n, 6, 128), generator=g).bfloat16()
    ws = torch.softmax(torch.randn((n, 6), generator=g), dim=1)
    if bank_dtype is None:
        return RetrievalIndex.from_features(feats, [ws], ids, group="tva", weights_softmaxed=True, groups=groups)
    mx = bank_dtype == "mxfp4"
    codes = torch.randint(0, 256, (n, 6, 64 if mx else 128), generator=g, dtype=torch.uint8)
    scales = torch.randint(100, 140, (n, 6, 4), generator=g, dtype=torch.uint8) if mx else torch.rand((n, 6), generator=g)
    index = RetrievalIndex("tva", "fine", False, [codes], [ws], ids, bank_dtype, scales=[scales], dtype=torch.bfloat16, exact="host",
                           exact_feats=[feats])
    index._append_groups(n, groups, before=0)
    return index


def _rows(index):
    """every per-row store of the index, as CPU tensors"""
    banks = index.feats + index.weights + (index.scales or []) + (index.exact_feats or [])
    return [b.cpu() for b in banks if b is not None]


def test_remove_and_live():
    index = _cpu_index()
    assert len(index) == 9 and index.live == 9 and index.alive is None and index.groups is None
    assert index.remove(ids=["clip2", "clip5"]) == 2
    assert index.remove(indices=[5, 7, 7]) == 1                        # 5 is gone already, 7 counts once
    assert index.remove(indices=torch.tensor([2])) == 0
    assert len(index) == 9 and index.live == 6
    assert index.alive.tolist() == [True, True, False, True, True, False, True, False, True]
    with pytest.raises(KeyError):
        index.remove(ids=["clip1", "nobody"])
    with pytest.raises(IndexError):
        index.remove(indices=[0, 9])
    with pytest.raises(ValueError):
        index.remove()
    with pytest.raises(ValueError):
        index.remove(ids=["clip1"], indices=[1])
    assert index.live == 6 and bool(index.alive[1]) and bool(index.alive[0])      # a refused call changes nothing
    # rows added later are alive, and removable by id
    index.add_features([index.feats[0][:2].clone()], [index.weights[0][:2].clone()], ["new0", "new1"])
    assert len(index) == 11 and index.live == 8 and index.alive.tolist()[9:] == [True, True]
    assert index.remove(ids=["new1"]) == 1 and index.alive.tolist()[9:] == [True, False]


@pytest.mark.parametrize("bank_dtype", [None, "fp8", "mxfp4"])
def test_compact_rewrites_every_store(bank_dtype):
    labels = ["a", "a", "b", None, "c", "c", "c", "d", "b"]
    index = _cpu_index(bank_dtype, labels)
    before, ids = _rows(index), list(index.ids)
    assert index.compact().tolist() == list(range(9))                  # nothing removed: the identity
    index.remove(indices=[0, 1, 4, 8])
    remap = index.compact()
    stay = [2, 3, 5, 6, 7]
    assert remap.dtype == torch.int64 and remap.tolist() == [-1, -1, 0, 1, -1, 2, 3, 4, -1]
    assert len(index) == 5 and index.live == 5 and index.alive is None and index.ids == [ids[j] for j in stay]
    for old, new in zip(before, _rows(index)):
        assert new.dtype == old.dtype and torch.equal(new, old[stay])
    # the label table is what an index built from the survivors would hold: "a" is gone, first appearance orders the rest
    assert index.group_labels == ["b", "c", "d"] and index.groups.tolist() == [0, -1, 1, 1, 2]
    if bank_dtype is None:                                             # (a quantised index quantises added rows on the device)
        fresh = _cpu_index(None, labels)
        built = type(index).from_features(fresh.feats[0][stay], [fresh.weights[0][stay]], [ids[j] for j in stay], group="tva",
                                          weights_softmaxed=True, groups=[labels[j] for j in stay])
        assert built.fingerprint() == index.fingerprint() and built.group_labels == index.group_labels
        assert torch.equal(built.groups, index.groups) and torch.equal(built.feats[0], index.feats[0])
        index.add_features([fresh.feats[0][:1]], [fresh.weights[0][:1]], ["again"], groups=["d"])      # the stores still grow
        assert len(index) == 6 and index.groups.tolist()[-1] == 2 and index.alive is None


def test_update_replaces_rows():
    index = _cpu_index(groups=["a", "a", "b", "b", "c", "c", "d", "d", "e"])
    f, w = index.feats[0][:2].clone() + 1, index.weights[0][:2].clone()
    assert index.update(["clip3", "clip4"], [f], [w], groups=["b", "z"]) == 2
    assert len(index) == 11 and index.live == 9 and index.ids[9:] == ["clip3", "clip4"]
    assert index.alive.tolist() == [True, True, True, False, False, True, True, True, True, True, True]
    assert torch.equal(index.feats[0][9:], f) and index.groups.tolist()[9:] == [1, 5] and index.group_labels[5] == "z"
    assert index.remove(ids=["clip3"]) == 1                            # the id names the old and the new position: one was alive
    with pytest.raises(KeyError):
        index.update(["nobody"], [f[:1]], [w[:1]])
    assert len(index) == 11
    # rows that add_features refuses leave the index as it was: nothing stays tombstoned without a replacement
    alive, live = index.alive.clone(), index.live
    with pytest.raises(ValueError):
        index.update(["clip0", "clip1"], [f[:, :3]], [w[:, :3]])      # another token count
    with pytest.raises(ValueError):
        index.update(["clip0", "clip1"], [f], [w], groups=["one label"])
    assert torch.equal(index.alive, alive) and index.live == live and len(index) == 11
    fresh = _cpu_index()
    with pytest.raises(ValueError):
        fresh.update(["clip0"], [f[:1, :3]], [w[:1, :3]])
    assert fresh.alive is None and fresh.live == 9
    remap = index.compact()
    assert remap.tolist() == [0, 1, 2, -1, -1, 3, 4, 5, 6, -1, 7] and index.ids[-1] == "clip4"


def test_group_label_table():
    from valor_amd.search import RetrievalIndex
    index = _cpu_index()
    f, w = index.feats[0][:3].clone(), index.weights[0][:3].clone()
    assert index.groups is None and index.group_labels == []
    index.add_features([f], [w], ["x0", "x1", "x2"], groups=["v7", ("v", 8), "v7"])      # the first labels: earlier rows get -1
    assert index.groups.dtype == torch.int32 and index.groups.tolist() == [-1] * 9 + [0, 1, 0]
    index.add_features([f], [w], ["y0", "y1", "y2"])                                       # no labels: -1
    index.add_features([f], [w], ["z0", "z1", "z2"], groups=[("v", 8), None, 12])
    assert index.groups.tolist()[12:] == [-1, -1, -1, 1, -1, 2] and index.group_labels == ["v7", ("v", 8), 12]
    with pytest.raises(ValueError):
        index.add_features([f], [w], ["q0", "q1", "q2"], groups=["one"])
    assert len(index) == 18
    with pytest.raises(ValueError):
        RetrievalIndex.from_features(f, [w], ["a", "b", "c"], group="tv", weights_softmaxed=True, groups=["g"])
    q = {"feat_t": torch.zeros((2, 5, 128), dtype=torch.bfloat16)}
    with pytest.raises(ValueError, match="groups"):                    # collapse needs groups; checked before the device is
        _cpu_index().search(None, q, 3, collapse=True)


@pytest.mark.parametrize("bank_dtype", [None, "fp8", "mxfp4"])
def test_save_load_round_trip_with_the_new_keys(tmp_path, bank_dtype):
    from valor_amd.search import RetrievalIndex
    index = _cpu_index(bank_dtype, ["a", "a", "b", None, "c", "c", "c", 4, "b"])
    index.remove(indices=[1, 6])
    index.save(tmp_path / "bank.pt")
    blob = torch.load(tmp_path / "bank.pt", weights_only=True)
    assert {"alive", "groups", "group_labels"} <= set(blob) and not {"alive", "groups", "group_labels"} & set(blob["fingerprint"])
    back = RetrievalIndex.load(tmp_path / "bank.pt", "cpu")
    assert back.fingerprint() == index.fingerprint() and back.ids == index.ids
    assert len(back) == 9 and back.live == 7 and torch.equal(back.alive, index.alive)
    assert torch.equal(back.groups, index.groups) and back.group_labels == ["a", "b", "c", 4]
    for a, b in zip(_rows(index), _rows(back)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert back.remove(ids=["clip0"]) == 1 and back.live == 6          # the loaded arrays are the index's own: they change and grow
    if bank_dtype is None:
        back.add_features([index.feats[0][:1]], [index.weights[0][:1]], ["more"], groups=["c"])
        assert back.groups.tolist()[-1] == 2 and back.alive.tolist()[-1] is True


@pytest.mark.parametrize("bank_dtype", [None, "fp8", "mxfp4"])
def test_files_without_the_new_keys_load(tmp_path, bank_dtype):
    """an index that removed nothing and has no groups writes the file it wrote before; so a file of the earlier formats, which has
    none of the keys, loads as it did"""
    from valor_amd.search import RetrievalIndex
    index = _cpu_index(bank_dtype)
    index.save(tmp_path / "plain.pt")
    blob = torch.load(tmp_path / "plain.pt", weights_only=True)
    want = {"format", "fingerprint", "ids", "weights"} | ({"feats"} if bank_dtype is None else {"codes", "scales", "exact_feats"})
    assert set(blob) == want
    assert blob["format"].endswith({None: "/1", "fp8": "/3", "mxfp4": "/5"}[bank_dtype])
    back = RetrievalIndex.load(tmp_path / "plain.pt", "cpu")
    assert back.alive is None and back.groups is None and back.group_labels == [] and back.live == len(back) == 9
    for a, b in zip(_rows(index), _rows(back)):
        assert torch.equal(a, b)
    # bad arrays are refused
    blob["alive"] = torch.ones(8, dtype=torch.bool)
    torch.save(blob, tmp_path / "bad.pt")
    with pytest.raises(ValueError):
        RetrievalIndex.load(tmp_path / "bad.pt", "cpu")
