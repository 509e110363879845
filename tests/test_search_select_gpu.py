"""Retrieval search with removal, filters and one result per group, on the GPU: valor_topk_rows_select (csrc/search_select.hip) against
its host statement topk_select_host, exactly, in values and indices; RetrievalIndex.remove / compact / where= / collapse= on every search
path against the host law applied to the index's own scores().

The index tests use exact-input banks: features in {-1, 0, 1}, D = 128, 4 tokens per side, unit token weights (0.25 after the softmax).
Every token similarity is an integer of magnitude <= 128 and every fine score a multiple of 1 / 8 below 2^7: exactly representable, so
no score depends on the order of a sum and equal scores occur by themselves (ten clips are copies of ten others besides)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _same(got, want):
    gv, gi = got[0].cpu(), got[1].cpu()
    wv, wi = want[0].cpu(), want[1].cpu()
    assert torch.equal(gi, wi), (gi, wi)
    assert torch.equal(torch.isnan(gv), torch.isnan(wv)) and torch.equal(torch.nan_to_num(gv, nan=0.0), torch.nan_to_num(wv, nan=0.0))


def _matrix(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((R, C), generator=g) * 8).round() / 8          # ties


def _on(dev, t):
    return None if t is None else t.to(dev)


def _check(dev, s, d, k, keep=None, group=None, base=0):
    from valor_amd.search import topk_rows_select, topk_select_host
    got = topk_rows_select(d, k, col_base=base, keep=_on(dev, keep), group=_on(dev, group))
    _same(got, topk_select_host(s, k, base=base, keep=keep, group=group))
    return got


# ------------------------------------------------------------------ 1. the kernel
def _patterns(R, C):
    """name -> (keep, group): the tables of one shape"""
    g = torch.Generator().manual_seed(100 * R + C)
    cols = torch.arange(C)
    all_but_one = torch.ones(C, dtype=torch.bool)
    all_but_one[C // 2] = False
    return {"keep none": (torch.zeros(C, dtype=torch.bool), None),
            "keep all but one": (all_but_one, None),
            "keep per row": (torch.rand((R, C), generator=g) < 0.5, None),
            "own groups": (None, torch.full((C,), -1, dtype=torch.int32)),
            "one group": (None, torch.full((C,), 3, dtype=torch.int32)),
            "groups of three": (None, (cols // 3).int()),
            "groups c % 5": (None, (cols % 5).int()),
            "keep and groups per row": (torch.rand((R, C), generator=g) < 0.7, torch.randint(-1, 40, (R, C), generator=g, dtype=torch.int32))}


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("C", [1, 7, 64, 257, 4099])
def test_kernel_equals_host_law(dev, R, C):
    """every pattern and every k in one case (a launch is microseconds); C = 4099 spans two column segments, so the members of a
    c % 5 group meet in the merge kernel"""
    from valor_amd.search import topk_host, topk_rows, topk_rows_select
    s = _matrix(R, C, 10 * R + C)
    d = s.to(dev)
    for k in (1, 3, 10, 64, 256):
        plain = topk_rows_select(d, k)                                 # neither table: valor_topk_rows bit for bit
        _same(plain, topk_host(s, k))
        _same(plain, topk_rows(d, k))
        for name, (keep, group) in _patterns(R, C).items():
            got = _check(dev, s, d, k, keep, group)
            if name == "keep none":
                assert bool((got[1] == -1).all()) and bool(torch.isinf(got[0]).all())
            if name == "one group":
                assert bool((got[1][:, 1:] == -1).all()) and bool((got[1][:, 0] >= 0).all())


@pytest.mark.parametrize("k", [256, 10])
def test_kernel_ramps_with_groups_of_two(dev, k):
    """one row of 50000 columns, groups of two. The ascending ramp refills the buffer at every step and every refill holds both
    members of its groups: a threshold read from a buffer that still holds duplicates would be too high and prune a group's only
    member. The descending ramp never refills after the first step; the third row puts equal values inside every group."""
    C = 50000
    ramp = torch.arange(C, dtype=torch.float32)[None]
    s = torch.cat((ramp, -ramp, (ramp / 2).floor(), _matrix(1, C, 5)), 0)
    group = (torch.arange(C) // 2).int()
    got = _check(dev, s, s.to(dev), k, None, group)
    assert got[1][0].tolist() == list(range(C - 1, C - 1 - 2 * k, -2))              # the better member of the k last groups
    assert got[1][1].tolist() == list(range(0, 2 * k, 2))
    assert got[1][2].tolist() == list(range(C - 2, C - 2 - 2 * k, -2))              # equal values: the lower index stands for the group
    keep = torch.ones(C, dtype=torch.bool)
    keep[1::2] = False                                                 # only the worse member of every group of the ascending ramp
    _check(dev, s, s.to(dev), k, keep, group)


def test_kernel_fewer_than_k_eligible_groups(dev):
    s = _matrix(5, 64, 7)
    group = (torch.arange(64) % 5).int()
    got = _check(dev, s, s.to(dev), 10, None, group)
    assert bool((got[1][:, :5] >= 0).all()) and bool((got[1][:, 5:] == -1).all()) and bool(torch.isinf(got[0][:, 5:]).all())
    keep = group != 2                                                  # a whole group ruled out: four results
    got = _check(dev, s, s.to(dev), 10, keep, group)
    assert bool((got[1][:, :4] >= 0).all()) and bool((got[1][:, 4:] == -1).all())
    assert sorted((got[1][0, :4] % 5).tolist()) == [0, 1, 3, 4]


def _folded(dev, d, k, step, keep, group, base=0, reverse=False):
    from valor_amd.search import topk_rows_select
    R, C = d.shape
    state = (torch.full((R, k), float("-inf"), device=dev), torch.full((R, k), -1, dtype=torch.int64, device=dev))
    starts = list(range(0, C, step))
    for c0 in (reversed(starts) if reverse else starts):
        topk_rows_select(d[:, c0:c0 + step], k, col_base=base + c0, state=state, keep=_on(dev, keep), group=_on(dev, group))
    return state


@pytest.mark.parametrize("C", [4099, 12345])
def test_kernel_streaming_equals_one_pass(dev, C):
    """chunks of 1000 columns folded with merge = 1, in either order, with large bases. Row 0: the best member of group 18 is in the
    last chunk and replaces the representative found before; row 1: the best member of group 0 is in the first chunk and every later
    member vanishes. The same holds without either table."""
    from valor_amd.search import topk_select_host
    s = _matrix(5, C, C)
    g = torch.Generator().manual_seed(2)
    group = (torch.arange(C) % 37).int()
    group[::11] = -1
    last = max(c for c in range(C - 100, C) if c % 37 == 18 and c % 11)
    s[0, last], s[1, 37] = 100.0, 100.0
    keep = torch.rand(C, generator=g) < 0.8
    keep[last], keep[37] = True, True
    keep_rows = torch.rand((5, C), generator=g) < 0.6
    d = s.to(dev)
    for k in (10, 256):
        for kp, gr in ((None, group), (keep, group), (keep_rows, None), (keep_rows, group), (None, None)):
            want = topk_select_host(s, k, keep=kp, group=gr)
            if gr is not None and kp is not keep_rows:
                assert want[1][0, 0] == last and want[1][1, 0] == 37
            _same(_folded(dev, d, k, 1000, kp, gr), want)
            _same(_folded(dev, d, k, 1000, kp, gr, reverse=True), want)
    # indices beyond 2^31: the tables are addressed by the index, so a shared table of that length is out of reach; per-row tables
    # are not needed for it either -- the plain selection through this entry covers the large base
    want = topk_select_host(s, 10, base=2 ** 33)
    _same(_folded(dev, d, 10, 1000, None, None, base=2 ** 33), want)
    # an entry of the state that the filter no longer admits drops out on the next merge
    from valor_amd.search import topk_rows_select
    state = _folded(dev, d, 10, 1000, keep, group)
    held = (state[0].cpu(), state[1].cpu())
    gone = keep.clone()
    gone[last] = False
    topk_rows_select(d[:, :0], 10, state=state, keep=gone.to(dev), group=group.to(dev))
    _same(state, topk_select_host(s[:, :0], 10, state=held, keep=gone, group=group))
    assert last in held[1][0].tolist() and last not in state[1][0].tolist()


def test_kernel_ties_within_and_across_groups(dev):
    """a block of equal values: inside a group the lowest index stands for it, equal representatives rank by index; NaN and -inf members"""
    s = torch.full((3, 1000), 0.25)
    group = (torch.arange(1000) // 4).int()
    got = _check(dev, s, s.to(dev), 64, None, group)
    assert torch.equal(got[1].cpu(), (4 * torch.arange(64))[None].expand(3, 64))
    keep = torch.ones(1000, dtype=torch.bool)
    keep[::4] = False                                                  # the lowest index of every group ruled out: the next one
    got = _check(dev, s, s.to(dev), 64, keep, group)
    assert torch.equal(got[1].cpu(), (4 * torch.arange(64) + 1)[None].expand(3, 64))
    g = torch.Generator().manual_seed(0)
    s = _matrix(5, 4099, 1)
    s[torch.rand(s.shape, generator=g) < 0.2] = float("nan")
    s[torch.rand(s.shape, generator=g) < 0.05] = float("-inf")
    s[3] = float("nan")                                                # a row of NaNs: the lowest index of every group
    s[4, 5:] = float("nan")
    s[4, :5] = torch.tensor([-0.0, 0.0, float("-inf"), 1.0, 0.0])
    for k in (10, 256):
        for group in ((torch.arange(4099) // 3).int(), (torch.arange(4099) % 300).int()):
            got = _check(dev, s, s.to(dev), k, None, group)
            assert int(got[1].max()) < 4099
    got = _check(dev, s, s.to(dev), 10, None, (torch.arange(4099) // 3).int())
    assert got[1][3].tolist() == list(range(0, 30, 3)) and got[1][4, :2].tolist() == [3, 0]


def test_kernel_refuses_bad_arguments_without_launching(dev):
    """VALOR_ERR_ARG on device pointers, and the outputs keep what they held"""
    from valor_amd import lib
    from valor_amd.search import topk_select_workspace_bytes
    so = lib.load()
    R, C, k = 4, 1000, 10
    score = torch.zeros((R, C), device=dev)
    keep, group = torch.ones(C, dtype=torch.bool, device=dev), torch.zeros(C + 1, dtype=torch.int32, device=dev)
    val, idx = torch.full((R, k), 7.0, device=dev), torch.full((R, k), 7, dtype=torch.int64, device=dev)
    nb = topk_select_workspace_bytes(R, C, k)
    ws = torch.empty((nb + 16,), dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()

    def rows(score=P(score), ld=C, R=R, C=C, base=0, k=k, keep=P(keep), keep_ld=0, group=P(group), group_ld=0, val=P(val), idx=P(idx), ws=P(ws),
             ws_bytes=nb):
        return so.valor_topk_rows_select(None, score, ld, R, C, base, k, 0, keep, keep_ld, group, group_ld, val, idx, ws, ws_bytes)

    assert rows(keep_ld=-1) == -1 and rows(group_ld=-1) == -1 and rows(group=P(group) + 2) == -1
    assert rows(score=None) == -1 and rows(val=None) == -1 and rows(idx=None) == -1 and rows(ws=None) == -1
    assert rows(ld=C - 1) == -1 and rows(k=0) == -1 and rows(k=257) == -1 and rows(R=-1) == -1
    assert rows(ws_bytes=nb - 1) == -1 and rows(ws=P(ws) + 8) == -1 and rows(score=P(score) + 2) == -1 and rows(idx=P(idx) + 4) == -1
    assert rows(base=-1) == -1 and rows(base=2 ** 63 - 1000) == -1
    torch.cuda.synchronize()
    assert bool((val == 7.0).all()) and bool((idx == 7).all())
    assert rows(R=0) == 0 and rows(group=P(group) + 4) == 0            # a 4-byte aligned group runs
    torch.cuda.synchronize()
    assert idx[:, 0].tolist() == [0, 0, 0, 0] and bool((idx[:, 1:] == -1).all())       # one group, equal values: index 0
    from valor_amd.search import topk_rows_select
    with pytest.raises(ValueError):                                    # the wrapper sizes the tables: col_base + C entries
        topk_rows_select(score, k, col_base=1, keep=keep)
    with pytest.raises(ValueError):
        topk_rows_select(score, k, group=group.long())
    # tables cut to the chunk while the state holds an earlier chunk's indices: refused, the merge would read outside them
    state = (torch.zeros((R, k), device=dev), torch.arange(2000, 2000 + k, device=dev)[None].expand(R, k).contiguous())
    with pytest.raises(ValueError, match="state holds index"):
        topk_rows_select(score, k, col_base=0, state=state, keep=keep)
    with pytest.raises(ValueError, match="state holds index"):
        topk_rows_select(score, k, col_base=0, state=state, group=group[:C].contiguous())


# ------------------------------------------------------------------ 2. the index on exact inputs
NB, NQ, TOK, D, TOPK = 300, 5, 4, 128, 10


@pytest.fixture(scope="module")
def case():
    """features in {-1, 0, 1}; clips 10 .. 19 are copies of clips 0 .. 9; 37 rows to remove; groups of 1 - 6 consecutive segments; the
    fp64 and the fp32 host scores of these inputs agree bit for bit (computed once)"""
    g = torch.Generator().manual_seed(21)
    fb = torch.randint(-1, 2, (NB, TOK, D), generator=g).float()
    fb[10:20] = fb[:10]
    fa = torch.randint(-1, 2, (NQ, TOK, D), generator=g).float()

    def host(dtype):
        x = torch.einsum("atd,bvd->abtv", fa.to(dtype), fb.to(dtype))
        return (0.25 * x.max(dim=3)[0].sum(-1) + 0.25 * x.max(dim=2)[0].sum(-1)) / 2.0

    exact = host(torch.float64)
    assert torch.equal(host(torch.float32).double(), exact) and torch.equal(exact.float().double(), exact)
    assert torch.equal(fb.bfloat16().float(), fb)
    best0 = int(exact[0].argmax())
    removed = torch.unique(torch.cat((torch.randperm(NB, generator=g)[:36], torch.tensor([best0]))))      # query 0's best clip among them
    while removed.numel() < 37:
        removed = torch.unique(torch.cat((removed, torch.randint(0, NB, (1,), generator=g))))
    labels, v = [], 0
    while len(labels) < NB:
        labels += [f"video{v}"] * int(torch.randint(1, 7, (1,), generator=g))
        v += 1
    labels = labels[:NB]
    where = torch.rand(NB, generator=g) < 0.4
    where_rows = torch.rand((NQ, NB), generator=g) < 0.3
    return dict(fa=fa.bfloat16(), fb=fb.bfloat16(), exact=exact.float(), removed=removed, best0=best0, labels=labels, where=where,
                where_rows=where_rows)


def _index(case, dev, bank_dtype=None, exact=None, groups=True):
    from valor_amd.search import RetrievalIndex
    index = RetrievalIndex.from_features(case["fb"].to(dev), None, [f"c{j}" for j in range(NB)], group="tv", bank_dtype=bank_dtype, exact=exact,
                                         groups=case["labels"] if groups else None)
    return index, {"feat_t": case["fa"].to(dev)}


def _no_repeats(groups):
    for row in groups.cpu().tolist():
        seen = [g for g in row if g >= 0]
        assert len(seen) == len(set(seen)), row


def test_plain_index_is_untouched(dev, case):
    """nothing removed, no groups, no where: what search() returned before these arguments existed"""
    from valor_amd.search import topk_host
    index, q = _index(case, dev, groups=False)
    sc = index.scores(None, q)
    assert torch.equal(sc.cpu(), case["exact"])                        # the exact inputs are exact on the device too
    for chunk in (None, 64):
        res = index.search(None, q, TOPK, chunk=chunk)
        _same((res.scores, res.indices), topk_host(sc, TOPK))
        assert bool((res.groups == -1).all()) and res.groups.dtype == torch.int32 and res.group_labels[0] == [None] * TOPK
    with pytest.raises(ValueError, match="groups"):
        index.search(None, q, TOPK, collapse=True)
    with pytest.raises(ValueError, match="where"):
        index.search(None, q, TOPK, where=torch.ones(NB - 1, dtype=torch.bool, device=dev))


@pytest.mark.parametrize("chunk", [None, 64])
def test_search_after_remove_and_compact(dev, case, chunk):
    from valor_amd.search import RetrievalIndex, topk_select_host
    index, q = _index(case, dev)
    removed = case["removed"]
    assert index.remove(indices=removed[:20]) == 20 and index.remove(ids=[f"c{j}" for j in removed[15:].tolist()]) == 17
    assert index.live == NB - 37 and len(index) == NB
    sc = index.scores(None, q, chunk=chunk)
    for k in (TOPK, 256):
        res = index.search(None, q, k, chunk=chunk)
        _same((res.scores, res.indices), topk_select_host(sc, k, keep=index.alive.cpu()))
        assert not set(res.indices.flatten().tolist()) & set(removed.tolist())
    assert case["best0"] in removed.tolist() and int(res.indices[0, 0]) != case["best0"]
    # explicit indices still read removed rows: the caller named them
    named = removed[None, :5].expand(NQ, 5).contiguous().to(dev)
    assert torch.equal(index.rescore(None, q, named).cpu(), case["exact"][:, removed[:5]])
    before = index.search(None, q, TOPK, chunk=chunk)
    remap = index.compact()
    assert remap.device == index.device and len(index) == index.live == NB - 37 and int((remap < 0).sum()) == 37
    stay = [j for j in range(NB) if j not in set(removed.tolist())]
    built = RetrievalIndex.from_features(case["fb"][stay].to(dev), None, [f"c{j}" for j in stay], group="tv", groups=[case["labels"][j] for j in stay])
    assert built.ids == index.ids and built.group_labels == index.group_labels and torch.equal(built.groups, index.groups)
    assert torch.equal(built.feats[0], index.feats[0]) and torch.equal(built.weights[0], index.weights[0])
    after, fresh = index.search(None, q, TOPK, chunk=chunk), built.search(None, q, TOPK, chunk=chunk)
    _same((after.scores, after.indices), (fresh.scores, fresh.indices))
    _same((after.scores, after.indices), (before.scores, remap[before.indices]))
    assert after.ids == before.ids


def _within_lists(where_rows, dev):
    """every query's admitted indices as one padded candidate matrix (-1 = nothing), shuffled: within= sorts them itself"""
    rows = [torch.nonzero(r).view(-1) for r in where_rows]
    width = max(r.numel() for r in rows)
    g = torch.Generator().manual_seed(4)
    out = torch.full((len(rows), width), -1, dtype=torch.int64)
    for a, r in enumerate(rows):
        out[a, :r.numel()] = r[torch.randperm(r.numel(), generator=g)]
    return out.to(dev)


def test_where_shared_and_per_query(dev, case):
    from valor_amd.search import topk_select_host
    index, q = _index(case, dev)
    index.remove(indices=case["removed"])
    sc, alive = index.scores(None, q), index.alive.cpu()
    for where in (case["where"], case["where_rows"]):
        for k in (TOPK, 256):
            res = index.search(None, q, k, chunk=64, where=where.to(dev))
            _same((res.scores, res.indices), topk_select_host(sc, k, keep=where & alive))
            rows = where if where.dim() == 2 else where[None].expand(NQ, NB)
            sub = index.search(None, q, k, within=_within_lists(rows, dev))           # its removed entries count as -1
            _same((sub.scores, sub.indices), (res.scores, res.indices))
            both = index.search(None, q, k, within=_within_lists(torch.ones((NQ, NB), dtype=torch.bool), dev), where=where.to(dev))
            _same((both.scores, both.indices), (res.scores, res.indices))
    nothing = index.search(None, q, TOPK, where=torch.zeros(NB, dtype=torch.bool, device=dev))
    assert bool((nothing.indices == -1).all()) and bool(torch.isinf(nothing.scores).all()) and nothing.ids[0] == [None] * TOPK


def _check_collapsed(res, sc, keep, index, case, k):
    """the host law, no group twice, every returned clip its group's best admitted segment, .groups / .group_labels"""
    from valor_amd.search import topk_select_host
    groups = index.groups.cpu()
    _same((res.scores, res.indices), topk_select_host(sc, k, keep=keep, group=groups))
    _no_repeats(res.groups)
    idx = res.indices.cpu()
    assert torch.equal(res.groups.cpu(), torch.where(idx >= 0, groups[idx.clamp(min=0)], torch.full_like(idx, -1, dtype=torch.int32)))
    assert res.group_labels == [[case["labels"][j] if j >= 0 else None for j in row] for row in idx.tolist()]
    sc = sc.cpu()
    for a in range(NQ):
        admitted = keep if keep is None or keep.dim() == 1 else keep[a]
        for j in idx[a].tolist():
            if j < 0:
                continue
            members = [m for m in torch.nonzero(groups == groups[j]).view(-1).tolist() if admitted is None or bool(admitted[m])]
            best = max(members, key=lambda m: (float(sc[a, m]), -m))
            assert best == j, (a, j, members)


def test_collapse_one_result_per_group(dev, case):
    index, q = _index(case, dev)
    sc = index.scores(None, q)
    for k in (TOPK, 256):
        for chunk in (None, 64):
            _check_collapsed(index.search(None, q, k, chunk=chunk, collapse=True), sc, None, index, case, k)
    index.remove(indices=case["removed"])
    alive = index.alive.cpu()
    _check_collapsed(index.search(None, q, TOPK, chunk=64, collapse=True), sc, alive, index, case, TOPK)
    for where in (case["where"], case["where_rows"]):
        res = index.search(None, q, TOPK, chunk=64, collapse=True, where=where.to(dev))
        _check_collapsed(res, sc, where & alive, index, case, TOPK)
        rows = where if where.dim() == 2 else where[None].expand(NQ, NB)
        sub = index.search(None, q, TOPK, within=_within_lists(rows, dev), collapse=True)
        _same((sub.scores, sub.indices), (res.scores, res.indices))
        assert torch.equal(sub.groups, res.groups)
    # explain alongside collapse: scores and indices bit for bit, the alignment of exactly those indices
    plain = index.search(None, q, TOPK, collapse=True)
    told = index.search(None, q, TOPK, collapse=True, explain=True)
    assert torch.equal(plain.scores, told.scores) and torch.equal(plain.indices, told.indices) and torch.equal(plain.groups, told.groups)
    assert plain.alignment is None and torch.equal(told.alignment.indices, told.indices)


def _two_stage_host(walk, exact, k, shortlist, keep, group):
    """search(shortlist=) on the host: the walk's `shortlist` best admitted clips (no collapsing), then the exact scores of those,
    collapsed"""
    from valor_amd.search import topk_select_host, within_finish, within_prepare
    cand = topk_select_host(walk, shortlist, keep=keep)[1]
    srt = within_prepare(cand, walk.shape[1])
    table = lambda t: (t[None].expand(srt.shape[0], -1) if t.dim() == 1 else t).gather(1, srt.clamp(min=0))
    if keep is not None:
        srt = torch.where(table(keep), srt, torch.full_like(srt, -1))
    pair = torch.where(srt >= 0, exact.gather(1, srt.clamp(min=0)), torch.full(srt.shape, float("-inf")))
    gpos = None if group is None else torch.where(srt >= 0, table(group), torch.full_like(srt, -1, dtype=torch.int32))
    return within_finish(*topk_select_host(pair, k, keep=srt >= 0, group=gpos), srt)


@pytest.mark.parametrize("bank_dtype", ["fp8", "mxfp4"])
def test_quantised_banks(dev, case, bank_dtype):
    """the three checks on codes alone (shortlist=0) against the host law on the bank's own scores(); then the two-stage search: the
    first stage filters and does not collapse, the second returns the exact scores, and no removed row survives either"""
    from valor_amd.search import topk_select_host
    index, q = _index(case, dev, bank_dtype, exact="device")
    index.remove(indices=case["removed"])
    removed = set(case["removed"].tolist())
    walk, alive, groups = index.scores(None, q).cpu(), index.alive.cpu(), index.groups.cpu()
    where = case["where_rows"]
    res = index.search(None, q, TOPK, chunk=64, shortlist=0)
    _same((res.scores, res.indices), topk_select_host(walk, TOPK, keep=alive))
    assert not set(res.indices.flatten().tolist()) & removed
    res = index.search(None, q, TOPK, chunk=64, shortlist=0, where=where.to(dev))
    _same((res.scores, res.indices), topk_select_host(walk, TOPK, keep=where & alive))
    res = index.search(None, q, TOPK, chunk=64, shortlist=0, collapse=True)
    _check_collapsed(res, walk, alive, index, case, TOPK)
    exact = index.rescore(None, q, torch.arange(NB, device=dev)[None].expand(NQ, NB).contiguous()).cpu()     # the store's own pair scores
    assert torch.equal(exact, case["exact"])
    for shortlist in (TOPK, 40, 256):
        for keep, kw in ((alive, {}), (where & alive, {"where": where.to(dev)})):
            for collapse in (False, True):
                res = index.search(None, q, TOPK, chunk=64, shortlist=shortlist, collapse=collapse, **kw)
                want = _two_stage_host(walk, exact, TOPK, shortlist, keep, groups if collapse else None)
                _same((res.scores, res.indices), want)
                idx = res.indices.cpu()
                assert not set(idx.flatten().tolist()) & removed
                got = torch.where(idx >= 0, exact.gather(1, idx.clamp(min=0)), torch.full(idx.shape, float("-inf")))
                assert torch.equal(res.scores.cpu(), got)              # the exact scores, not the walk's
                if collapse:
                    _no_repeats(res.groups)
    # the shortlist counts segments: with k of them a collapsed result holds fewer than k groups, a larger one fills it
    few = index.search(None, q, TOPK, shortlist=TOPK, collapse=True)
    full = index.search(None, q, TOPK, shortlist=256, collapse=True)
    assert int((few.indices >= 0).sum()) <= int((full.indices >= 0).sum()) == NQ * TOPK


def test_save_and_load_on_the_device(dev, case, tmp_path):
    from valor_amd.search import RetrievalIndex, topk_select_host
    index, q = _index(case, dev)
    index.remove(indices=case["removed"])
    index.save(tmp_path / "bank.pt")
    back = RetrievalIndex.load(tmp_path / "bank.pt", dev)
    assert back.live == NB - 37 and torch.equal(back.alive, index.alive) and torch.equal(back.groups, index.groups)
    assert back.group_labels == index.group_labels and back.alive.device == back.device
    sc = back.scores(None, q)
    for collapse in (False, True):
        a, b = index.search(None, q, TOPK, collapse=collapse), back.search(None, q, TOPK, collapse=collapse)
        _same((b.scores, b.indices), (a.scores, a.indices))
        _same((b.scores, b.indices), topk_select_host(sc, TOPK, keep=back.alive.cpu(), group=back.groups.cpu() if collapse else None))
        assert not set(b.indices.flatten().tolist()) & set(case["removed"].tolist())
        assert b.group_labels == a.group_labels
    _no_repeats(b.groups)
    # update: the replaced rows answer from their new positions
    old = torch.nonzero(back.alive).view(-1)[:3].tolist()
    assert back.update([f"c{j}" for j in old], [case["fb"][old].to(dev)], [back.weights[0][old].clone()], groups=[case["labels"][j] for j in old]) == 3
    assert len(back) == NB + 3 and back.live == NB - 37
    where = torch.zeros(NB + 3, dtype=torch.bool, device=dev)
    where[old + [NB, NB + 1, NB + 2]] = True
    res = back.search(None, q, TOPK, where=where)
    assert [sorted(row[:3]) for row in res.indices.tolist()] == [[NB, NB + 1, NB + 2]] * NQ and bool((res.indices[:, 3:] == -1).all())
    assert res.ids[0][3:] == [None] * (TOPK - 3) and sorted(res.ids[0][:3]) == sorted(f"c{j}" for j in old)
