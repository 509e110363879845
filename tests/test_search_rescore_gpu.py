"""Pair scores on the GPU (csrc/search_pairs.hip) and what stands on them in search.RetrievalIndex: rescore, search(within=), the
exact store of an fp8 bank and the two-stage search.

valor_fine_score_pairs is held to pair_scores_host (fp64 on the bf16 features) inside the band the project grants the fused score path,
2e-5 + 1e-5 |s| (tests/test_search_gpu.py, tests/test_evaluate_gpu.py), and to valor_fine_fused_fwd on the same pairs inside the same
band (whether the two agree bit for bit is printed, not asserted: DESIGN.md section 3.4 records the answer). Everything the index does
on top is integer work on those scores and is held to the host plan exactly."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ATOL, RTOL = 2e-5, 1e-5


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _soft(raw, mask):
    return torch.softmax(raw.masked_fill(mask == 0, float("-inf")), dim=-1)


def _in_band(got, want):
    err = (got.double() - want.double()).abs()
    return err, bool((err <= ATOL + RTOL * want.double().abs()).all())


# ------------------------------------------------------------------ 1. the kernel
NS = 50


def _kernel_case(NA, C, T, Nv, D, seed):
    """queries whose first text points AWAY from every clip (all its dot products negative, so the 0 of a masked token wins max_t, as
    the law says), masks with trailing zeros, non-uniform weights; candidate rows with -1, NS, 2^40, a duplicate, unsorted"""
    g = torch.Generator().manual_seed(seed)
    u = _unit(torch.randn((D,), generator=g))
    store = _unit(_unit(torch.randn((NS, Nv, D), generator=g)) + 0.7 * u).bfloat16()
    fa = _unit(torch.randn((NA, T, D), generator=g))
    fa[0] = _unit(fa[0] - 1.5 * u)
    fa = fa.bfloat16()
    lens = torch.randint(1, T + 1, (NA,), generator=g)
    lens[0] = max(1, T - 2)
    mask = (torch.arange(T)[None] < lens[:, None]).float()
    wa, ws = _soft(torch.randn((NA, T), generator=g), mask), torch.softmax(2 * torch.randn((NS, Nv), generator=g), -1)
    cand = torch.randint(0, NS, (NA, C), generator=g)
    if C >= 7:
        cand[:, 1], cand[:, 2], cand[:, 3], cand[:, 4] = -1, NS, 1 << 40, cand[:, 0]
        cand[:, 5], cand[:, 6] = NS - 1, 0
    else:
        cand[:, 0] = torch.tensor([NS - 1, -1, NS])[:NA]
    return fa, mask, wa, store, ws, cand


@pytest.mark.parametrize("Nv", [1, 10, 17, 64])
@pytest.mark.parametrize("T", [1, 5, 16, 33, 64])
def test_pair_kernel_against_the_host_law_and_the_fused_kernel(dev, T, Nv):
    from valor_amd import kernels as K, lib
    from valor_amd.search import pair_scores_host
    worst, identical, negative_won = 0.0, True, False
    for D in (64, 512):
        for NA in (1, 3):
            for C in (1, 7, 33):
                fa, mask, wa, store, ws, cand = _kernel_case(NA, C, T, Nv, D, seed=1000 * T + 10 * Nv + NA + C)
                want = pair_scores_host(fa, mask, wa, store, ws, cand)
                ok = (cand >= 0) & (cand < NS)
                d = [t.to(dev).contiguous() for t in (fa, mask, wa, store, ws)]
                ld_c, ld_s = C + 2, C + 3                              # both rows wider than C: only C columns are read / written
                cand_d = torch.full((NA, ld_c), 1 << 50, dtype=torch.int64, device=dev)
                cand_d[:, :C] = cand.to(dev)
                out = torch.full((NA, ld_s), 123.0, device=dev)
                lib.call("valor_fine_score_pairs", K._stream(), *[t.data_ptr() for t in d], NS, cand_d.data_ptr(), ld_c, out.data_ptr(), ld_s,
                         NA, C, T, Nv, D)
                got = out.cpu()
                assert bool((got[:, C:] == 123.0).all()), "columns beyond C were written"
                assert bool((got[:, :C][~ok] == float("-inf")).all()), "an out-of-range candidate must score exactly -inf"
                err, inside = _in_band(got[:, :C][ok], want[ok])
                worst = max(worst, float(err.max()) if err.numel() else 0.0)
                assert inside, (D, NA, C, float(err.max()))
                # the fused kernel on the same pairs: the full [NA, NS] matrix, gathered
                full = torch.full((NA, NS), float("nan"), device=dev)
                ones = torch.ones((NS, Nv), device=dev)
                lib.call("valor_fine_fused_fwd", K._stream(), d[0].data_ptr(), d[3].data_ptr(), d[1].data_ptr(), ones.data_ptr(), d[2].data_ptr(),
                         d[4].data_ptr(), full.data_ptr(), None, None, None, None, NA, NS, T, Nv, D)
                fused = full.cpu().gather(1, cand.clamp(0, NS - 1))
                err, inside = _in_band(got[:, :C][ok], fused[ok])
                assert inside, ("against valor_fine_fused_fwd", D, NA, C, float(err.max()))
                identical = identical and torch.equal(got[:, :C][ok], fused[ok])
                negative_won = negative_won or (T > 2 and bool((want[0][ok[0]] < 0).any()))
    print(f"T {T} Nv {Nv}: largest |kernel - host law| {worst:.3g}; bit-identical to valor_fine_fused_fwd on the same pairs: {identical}")
    if T > 2:
        assert negative_won, "the case must hold pairs of negative score (real negatives under the 0 of a masked token)"


@pytest.mark.parametrize("T,Nv,D", [(64, 10, 1024), (5, 17, 4096)])
def test_pair_kernel_stages_a_long_query_in_segments(dev, T, Nv, D):
    """a query image above 64 KiB of LDS (D > 32768 / padded T) goes through LDS in segments along D, restaged per round of candidates:
    two segments here, 33 candidates = three workgroups of up to four rounds"""
    from valor_amd.search import pair_scores_host, score_pairs
    NA, C = 2, 33
    fa, mask, wa, store, ws, cand = _kernel_case(NA, C, T, Nv, D, seed=T + D)
    want = pair_scores_host(fa, mask, wa, store, ws, cand)
    ok = (cand >= 0) & (cand < NS)
    got = score_pairs(*[t.to(dev).contiguous() for t in (fa, mask, wa, store, ws, cand)]).cpu()
    assert bool((got[~ok] == float("-inf")).all())
    err, inside = _in_band(got[ok], want[ok])
    print(f"T {T} Nv {Nv} D {D}: largest |kernel - host law| {float(err.max()):.3g}")
    assert inside, float(err.max())


def test_pair_kernel_reads_clips_past_two_gib_of_store(dev):
    """a store of 2.16 GB (33 000 clips of 64 tokens x 512): the last clips lie past byte offset 2^31, where a 32-bit offset would wrap.
    Only the rows the candidates name are filled (and known to the host law, which sees them as a store of four)."""
    from valor_amd.search import pair_scores_host, score_pairs
    big, Nv, D, T, NA = 33000, 64, 512, 5, 2
    fa, mask, wa, rows, ws, _ = _kernel_case(NA, 7, T, Nv, D, seed=9)
    rows, ws = rows[:4], ws[:4]
    where = torch.tensor([big - 1, big - 2, 32768, 0])                   # 32768 * 65536 bytes = 2^31 exactly
    store = torch.empty((big, Nv, D), dtype=torch.bfloat16, device=dev)
    wstore = torch.zeros((big, Nv), device=dev)
    store[where.to(dev)], wstore[where.to(dev)] = rows.to(dev), ws.to(dev)
    local = torch.tensor([[0, 1, 2, 3, -1, 4, 1], [3, 2, 1, 0, 0, -1, 4]])        # 4 = outside the store
    cand = torch.where((local >= 0) & (local < 4), where[local.clamp(0, 3)], torch.where(local < 0, local, torch.full_like(local, big)))
    want = pair_scores_host(fa, mask, wa, rows, ws, local)
    got = score_pairs(*[t.to(dev).contiguous() for t in (fa, mask, wa)], store, wstore, cand.to(dev)).cpu()
    ok = (local >= 0) & (local < 4)
    assert bool((got[~ok] == float("-inf")).all())
    err, inside = _in_band(got[ok], want[ok])
    assert inside, float(err.max())


def test_pair_kernel_refuses_bad_arguments_and_launches_nothing(dev):
    from valor_amd import kernels as K, lib
    so = lib.load()
    NA, C, T, Nv, D = 2, 7, 6, 10, 128
    fa, mask, wa, store, ws, cand = [t.to(dev).contiguous() for t in _kernel_case(NA, C, T, Nv, D, seed=5)]
    out = torch.full((NA, C), 123.0, device=dev)

    def score(**kw):
        a = dict(fa=fa.data_ptr(), ld_cand=C, T=T, D=D)
        a.update(kw)
        return so.valor_fine_score_pairs(K._stream(), a["fa"], mask.data_ptr(), wa.data_ptr(), store.data_ptr(), ws.data_ptr(), NS, cand.data_ptr(),
                                         a["ld_cand"], out.data_ptr(), C, NA, C, a["T"], Nv, a["D"])

    assert score(fa=None) == -1 and score(D=96) == -1 and score(T=65) == -1 and score(ld_cand=C - 1) == -1
    torch.cuda.synchronize()
    assert bool((out == 123.0).all())
    assert score() == 0
    torch.cuda.synchronize()
    assert not bool((out == 123.0).any())


# ------------------------------------------------------------------ 2. the index
NB, NV, T, D, NQ, TOPK = 300, 4, 6, 128, 5, 5


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(21)
    fb = _unit(torch.randn((NB, NV, D), generator=g)).bfloat16()
    fa = _unit(torch.randn((NQ, T, D), generator=g)).bfloat16()
    mask = (torch.arange(T)[None] < torch.randint(3, T + 1, (NQ, 1), generator=g)).float()
    wa, wb = torch.randn((NQ, T), generator=g), torch.randn((NB, NV), generator=g)
    subset = torch.stack([torch.randperm(NB, generator=g)[:40] for _ in range(NQ)])
    subset[:, 7], subset[:, 30], subset[:, 12] = subset[:, 3], subset[:, 3], -1     # repeats and a -1
    return dict(fa=fa, fb=fb, mask=mask, wa=wa, wb=wb, subset=subset)


def _queries(c, dev):
    return {"feat_t": c["fa"].to(dev), "mask": c["mask"].to(dev), "weight": c["wa"].to(dev)}


def _index(c, dev, bank_dtype=None, exact=None):
    from valor_amd.search import RetrievalIndex
    return RetrievalIndex.from_features(c["fb"].to(dev), c["wb"].to(dev), [f"c{j}" for j in range(NB)], group="tv", bank_dtype=bank_dtype, exact=exact)


def test_rescore_equals_the_index_scores_gathered(dev, case):
    index, q = _index(case, dev), _queries(case, dev)
    cand = case["subset"].to(dev)
    got = index.rescore(None, q, cand)
    assert got.shape == (NQ, 40) and got.dtype == torch.float32
    full = index.scores(None, q)
    ok = cand >= 0
    assert bool((got[~ok] == float("-inf")).all())
    err, inside = _in_band(got[ok].cpu(), full.gather(1, cand.clamp(min=0))[ok].cpu())
    print(f"largest |rescore - scores gathered| {float(err.max()):.3g}")
    assert inside


def test_rescore_adds_the_parts_of_a_late_fusion_bank(dev, case):
    from valor_amd.search import RetrievalIndex
    fv, fa = case["fb"][:, :2].contiguous().to(dev), case["fb"][:, 2:].contiguous().to(dev)
    index = RetrievalIndex.from_features([fv, fa], group="tva", late_fusion=True)
    q = {"feat_t": case["fa"].to(dev), "mask": case["mask"].to(dev)}
    cand = case["subset"].to(dev)
    got, full = index.rescore(None, q, cand), index.scores(None, q)
    ok = cand >= 0
    err = (got[ok] - full.gather(1, cand.clamp(min=0))[ok]).abs().cpu().double()
    assert bool((err <= 2 * (ATOL + RTOL * full.abs().max().item())).all())          # two parts: twice the band


@pytest.mark.parametrize("k", [5, 40])
def test_search_within_equals_the_host_plan_on_its_own_scores(dev, case, k):
    from valor_amd.search import topk_host, within_finish, within_prepare
    index, q = _index(case, dev), _queries(case, dev)
    cand = case["subset"].to(dev)
    res = index.search(None, q, k, within=cand)
    srt = within_prepare(case["subset"], NB)
    pair = index.rescore(None, q, srt.to(dev)).cpu()
    want_v, want_i = within_finish(*topk_host(pair, k), srt)
    assert torch.equal(res.indices.cpu(), want_i) and torch.equal(res.scores.cpu(), want_v)
    for row, members in zip(res.indices.cpu().tolist(), case["subset"].tolist()):
        assert all(j in members for j in row)
    if k == 40:                                                         # 37 distinct clips per list: the rest is -inf / -1
        assert bool((res.indices[:, 37:] == -1).all()) and bool((res.scores[:, 37:] == float("-inf")).all()) and bool((res.indices[:, :37] >= 0).all())
    assert res.ids[0] == [f"c{j}" if j >= 0 else None for j in want_i[0].tolist()]


def test_two_stage_search_with_both_stores(dev, case):
    from valor_amd.search import topk_host, within_finish, within_prepare
    q = _queries(case, dev)
    on_dev, on_host = _index(case, dev, "fp8", "device"), _index(case, dev, "fp8", "host")
    short = on_dev.search(None, q, 20, shortlist=0)                     # the fp8 walk alone
    plain = _index(case, dev, "fp8").search(None, q, 20)
    assert torch.equal(short.indices, plain.indices) and torch.equal(short.scores, plain.scores)
    srt = within_prepare(short.indices, NB)
    exact = on_dev.rescore(None, q, srt)
    want_v, want_i = within_finish(*topk_host(exact.cpu(), TOPK), srt.cpu())
    for index in (on_dev, on_host):
        res = index.search(None, q, TOPK, shortlist=20)
        assert torch.equal(res.indices.cpu(), want_i) and torch.equal(res.scores.cpu(), want_v)
    assert torch.equal(on_host.rescore(None, q, srt), exact)
    default = on_dev.search(None, q, TOPK)                              # shortlist None: min(256, 4 k) = 20
    assert torch.equal(default.indices.cpu(), want_i) and torch.equal(default.scores.cpu(), want_v)
    # the exact scores are those of the bf16 bank, within the band
    err, inside = _in_band(exact.cpu(), _index(case, dev).scores(None, q).gather(1, srt).cpu())
    assert inside, float(err.max())


def _planted_case(seed):
    """For each query five planted clips (noisy copies of the query's first tokens) whose exact scores lead the rest of the bank by at
    least 0.05 and differ among themselves by 2e-4 .. 1e-3: out of 400 noisy copies per query, a chain of five whose consecutive exact
    score gaps lie inside [2.5e-4, 9e-4]. All on the CPU, in fp64 on the bf16 features."""
    from valor_amd.search import pair_scores_host
    g = torch.Generator().manual_seed(seed)
    fb = _unit(torch.randn((NB, NV, D), generator=g)).bfloat16()
    fa = _unit(torch.randn((NQ, T, D), generator=g)).bfloat16()
    mask = (torch.arange(T)[None] < torch.randint(4, T + 1, (NQ, 1), generator=g)).float()
    wa_raw, wb_raw = torch.randn((NQ, T), generator=g), torch.randn((NB, NV), generator=g)
    wa, wb = _soft(wa_raw, mask), torch.softmax(wb_raw, -1)
    slots = torch.randperm(NB, generator=g)[:NQ * 5].view(NQ, 5)
    for i in range(NQ):
        sigma = 0.3 + 0.3 * torch.rand((400, 1, 1), generator=g)
        pool = _unit(fa[i, :NV].float()[None] + sigma * torch.randn((400, NV, D), generator=g) / D ** 0.5).bfloat16()
        w = wb[slots[i, 0]][None].expand(400, NV).contiguous()          # one weight row for the five: only the features differ
        s = pair_scores_host(fa[i:i + 1], mask[i:i + 1], wa[i:i + 1], pool, w, torch.arange(400)[None])[0]
        order = torch.argsort(s, descending=True).tolist()
        chain = []
        for start in range(len(order)):                                 # the first chain of five, from the best copy down
            chain = [order[start]]
            for j in order[start + 1:]:
                gap = float(s[chain[-1]] - s[j])
                if 2.5e-4 <= gap <= 9e-4:
                    chain.append(j)
                if len(chain) == 5 or gap > 9e-4:
                    break
            if len(chain) == 5:
                break
        assert len(chain) == 5, "no chain of five in the pool"
        fb[slots[i]] = pool[chain]
        wb_raw[slots[i]] = wb_raw[slots[i, 0]].clone()
    wb = torch.softmax(wb_raw, -1)
    exact = pair_scores_host(fa, mask, wa, fb, wb, torch.arange(NB)[None].expand(NQ, NB))
    return dict(fa=fa, fb=fb, mask=mask, wa=wa_raw, wb=wb_raw, wa_soft=wa, wb_soft=wb, slots=slots, exact=exact)


PLANTED_SEED = 0


def test_planted_clips_the_fp8_bank_misorders_and_the_two_stage_search_restores(dev):
    from valor_amd.search import fp8_scores_host, quantize_rows_host, topk_host
    c = _planted_case(PLANTED_SEED)
    exact, slots = c["exact"], c["slots"]
    # the construction holds: the planted five lead by 0.05, in steps of 2e-4 .. 1e-3 (above twice the band, below the quantisation error)
    want_v, want_i = topk_host(exact.float(), TOPK)
    rest = exact.clone()
    rest.scatter_(1, slots, float("-inf"))
    planted = exact.gather(1, slots)
    assert bool((planted.min(1)[0] - rest.max(1)[0] >= 0.05).all())
    gaps = -torch.diff(torch.sort(planted, dim=1, descending=True)[0], dim=1)
    assert bool((gaps >= 2e-4).all()) and bool((gaps <= 1e-3).all()) and 2e-4 > 2 * (ATOL + RTOL * float(planted.max()))
    assert sorted(want_i[0].tolist()) == sorted(slots[0].tolist())
    # the host restatement of the fp8 bank mis-orders the five for at least one query: otherwise the case shows nothing
    ca, sa = quantize_rows_host(c["fa"])
    cb, sb = quantize_rows_host(c["fb"])
    fp8 = fp8_scores_host(ca, sa, cb, sb, c["mask"], torch.ones((NB, NV)), c["wa_soft"], c["wb_soft"])
    fp8_i = topk_host(fp8.float(), TOPK)[1]
    wrong = [i for i in range(NQ) if fp8_i[i].tolist() != want_i[i].tolist()]
    print(f"the host law of the fp8 bank mis-orders the planted five of queries {wrong}; largest |fp8 - exact| {float((fp8 - exact).abs().max()):.3g}")
    assert wrong

    q = _queries(c, dev)
    bf16 = _index(c, dev)
    truth = bf16.search(None, q, TOPK).indices.cpu()
    assert torch.equal(truth, want_i)
    for store in ("device", "host"):
        two = bf16.quantize(exact=store)
        assert torch.equal(two.search(None, q, TOPK, shortlist=20).indices.cpu(), truth)
        alone = two.search(None, q, TOPK, shortlist=0).indices.cpu()
        assert any(alone[i].tolist() != truth[i].tolist() for i in range(NQ))


def test_host_store_keeps_no_bf16_copy_on_the_device_and_grows(dev, case):
    q = _queries(case, dev)
    whole = _index(case, dev, "fp8", "device")
    from valor_amd.search import RetrievalIndex
    head = RetrievalIndex.from_features(case["fb"][:200].to(dev), case["wb"][:200].to(dev), [f"c{j}" for j in range(200)], group="tv")
    index = head.quantize(exact="host")
    store = index.exact_feats[0]
    assert store.device.type == "cpu" and store.is_pinned() and store.dtype == torch.bfloat16 and store.shape == (200, NV, D)
    device_tensors = index.feats + index.scales + index.weights
    assert all(t.is_cuda for t in device_tensors) and [t.dtype for t in device_tensors] == [torch.uint8, torch.float32, torch.float32]
    assert index.bank_bytes() == 200 * NV * (D + 8) and index.fingerprint()["exact"] == "host"
    index.add_features([case["fb"][200:].to(dev)], [whole.weights[0][200:]], [f"c{j}" for j in range(200, NB)])
    assert len(index) == NB and index.exact_feats[0].shape[0] == NB and index.exact_feats[0].is_pinned()
    assert torch.equal(index.exact_feats[0], case["fb"]) and torch.equal(index.feats[0], whole.feats[0])
    new = torch.arange(200, NB, device=dev)[None].expand(NQ, NB - 200).contiguous()
    assert torch.equal(index.rescore(None, q, new), whole.rescore(None, q, new))
    a, b = index.search(None, q, TOPK, within=new), whole.search(None, q, TOPK, within=new)
    assert torch.equal(a.indices, b.indices) and torch.equal(a.scores, b.scores) and bool((a.indices >= 200).all())
    a, b = index.search(None, q, TOPK), whole.search(None, q, TOPK)
    assert torch.equal(a.indices, b.indices) and torch.equal(a.scores, b.scores)


@pytest.mark.parametrize("store", ["device", "host"])
def test_format_3_reloads_to_the_same_search(dev, case, tmp_path, store):
    from valor_amd.search import RetrievalIndex
    index, q = _index(case, dev, "fp8", store), _queries(case, dev)
    res = index.search(None, q, TOPK, shortlist=20)
    index.save(tmp_path / "bank3.pt")
    back = RetrievalIndex.load(tmp_path / "bank3.pt", dev)
    assert back.exact == store and back.fingerprint() == index.fingerprint() and back.exact_feats[0].is_cuda == (store == "device")
    again = back.search(None, q, TOPK, shortlist=20)
    assert torch.equal(again.indices, res.indices) and torch.equal(again.scores, res.scores) and again.ids == res.ids
