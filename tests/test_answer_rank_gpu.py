"""Exact ranking of a whole closed answer set by level-batched trie scoring. The kernel alone first (valor_trie_score_level against
decode.trie_level_host bit for bit, with the log-sum-exp handed in and computed in the launch; the argument errors), then
decode.rank_candidates on the small synthetic fp32 model of tests/test_answer_set_decode_gpu.py (its helpers restated): against the
teacher-forced fp64 re-run path, chunked and sub-batched, against an exhaustive beam search, top-k, 'lm', sample_num,
validate_qa(answer_ranking='exact') with planted answers, one bf16 run, and what the call leaves behind."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

EOS = 102
TERM = 5e-5                                 # per term of a score against the re-run path: the band of tests/test_answer_set_decode_gpu.py


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the kernel alone
def kernel_set(V):
    """a root with 300 children (more than one workgroup's threads) among them V - 1, leaves, a terminal node with a child ([201]), a
    node that is no answer ([201 9]), a candidate that is a prefix of another, a duplicate"""
    from valor_amd import decode
    firsts = list(range(200, 499)) + [V - 1]
    cands = [[t] for t in firsts] + [[200, 7], [200, 7, V - 1], [201, 9, 10], [200, 7]]
    return decode.AnswerSet(cands, vocab=V)


def level_rows(V, ld, n, b, dev, seed):
    """fp32 logits [n * b, V] inside a zero [n * b, ld] buffer"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.zeros((n * b, ld), device=dev)
    z = buf[:, :V]
    z.copy_((torch.randn((n * b, V), generator=g) * 2.0).to(dev))
    return z


@pytest.mark.parametrize("V,ld", [(1200, 1216), (1201, 1201)])
def test_kernel_equals_the_host_law_bit_for_bit(dev, V, ld):
    """lse from valor_xent_fwd; every level of the set, b = 3; what a level does not own keeps its NaN canary"""
    from valor_amd import decode, kernels as K
    b = 3
    a = kernel_set(V)
    lv, trie = a.levels(), a.device(dev)
    N = a.n_nodes
    ns = torch.full((N * b,), float("nan"), device=dev)
    fin = torch.full((N * b,), float("nan"), device=dev)
    ns.view(N, b)[int(a.root[0])] = 0.0
    assert lv.width == 300 and lv.depth_max == 3
    for d in range(lv.depth_max + 1):
        nodes = lv.order[lv.level_ptr[d]:lv.level_ptr[d + 1]]
        z = level_rows(V, ld, nodes.numel(), b, dev, seed=10 + d)
        assert z.stride(0) == ld and (ld % 4 == 0) == (V == 1200)
        lse = decode.row_lse(z)[0]
        want_ns, want_fin = decode.trie_level_host(z, lse, nodes, b, a, EOS, ns, fin)
        keep = z.clone()
        K.trie_score_level(z, nodes.to(dev), b, EOS, trie, ns, fin, lse=lse)
        assert same_bits(ns.cpu(), want_ns) and same_bits(fin.cpu(), want_fin), d
        assert same_bits(z, keep)                                                   # the logits are never written
    got = fin.view(N, b)[lv.cand_node.to(dev)].cpu()
    assert not torch.isnan(got).any()
    assert torch.isnan(fin.view(N, b)[(~a.terminal.bool()).to(dev)]).all()          # the root and [201 9]: no answer ends there
    assert int((~a.terminal.bool()).sum()) == 2 and same_bits(got[-1], got[-4])     # the duplicate [200 7]: equal scores
    # an index outside the trie in the level's node list is never dereferenced: the row writes nothing
    ns2, fin2 = ns.clone(), fin.clone()
    bad = torch.tensor([N + 5, -1], dtype=torch.int32, device=dev)
    K.trie_score_level(level_rows(V, ld, 2, b, dev, seed=3), bad, b, EOS, trie, ns2, fin2)
    assert same_bits(ns2, ns) and same_bits(fin2, fin)


def test_kernel_log_sum_exp_in_the_launch(dev):
    """lse null: lse_out against the fp64 log-sum-exp of the same fp32 rows, within twice the largest error valor_xent_fwd's own lse shows
    on those rows (measured here, printed); the scores are then the host law applied to lse_out, bit for bit"""
    from valor_amd import decode, kernels as K
    b = 3
    for V, ld in ((1200, 1216), (1201, 1201)):
        a = kernel_set(V)
        lv, trie = a.levels(), a.device(dev)
        N = a.n_nodes
        nodes = lv.order[lv.level_ptr[1]:lv.level_ptr[2]]                          # the 300 nodes of level 1: 900 rows
        z = level_rows(V, ld, nodes.numel(), b, dev, seed=21)
        ref = torch.logsumexp(z.cpu().double(), 1)
        xent = decode.row_lse(z)[0].cpu().double()
        err_x = float((xent - ref).abs().max())
        g = torch.Generator().manual_seed(4)
        ns = (torch.randn(N * b, generator=g) * 3.0).to(dev)
        fin = torch.full((N * b,), float("nan"), device=dev)
        ns0, fin0 = ns.clone(), fin.clone()
        lse_out = torch.full((z.shape[0],), float("nan"), device=dev)
        K.trie_score_level(z, nodes.to(dev), b, EOS, trie, ns, fin, lse_out=lse_out)
        err_k = float((lse_out.cpu().double() - ref).abs().max())
        print(f"V={V} ld={ld}: max |lse - fp64| valor_xent_fwd {err_x:.3e}, valor_trie_score_level {err_k:.3e} (band {2 * err_x:.3e})")
        assert err_x > 0 and err_k <= 2 * err_x
        want_ns, want_fin = decode.trie_level_host(z, lse_out, nodes, b, a, EOS, ns0, fin0)
        assert same_bits(ns.cpu(), want_ns) and same_bits(fin.cpu(), want_fin)
        ns1, fin1 = ns0.clone(), fin0.clone()                                       # lse_out is optional
        K.trie_score_level(z, nodes.to(dev), b, EOS, trie, ns1, fin1)
        assert same_bits(ns1, ns) and same_bits(fin1, fin)


def test_kernel_argument_errors_come_before_any_launch(dev):
    from valor_amd import kernels as K, lib
    V, ld, b = 1200, 1216, 3
    a = kernel_set(V)
    lv, t = a.levels(), a.device(dev)
    N, E = a.n_nodes, int(a.child_tok.numel())
    nodes = lv.order[1:3].to(dev)
    z = level_rows(V, ld, 2, b, dev, seed=1)
    ns = torch.full((N * b,), float("nan"), device=dev)
    fin = torch.full((N * b,), float("nan"), device=dev)
    p = lambda x: x.data_ptr()
    good = dict(logits=p(z), ld=ld, rows=2 * b, V=V, b=b, level_node=p(nodes), lse=None, lse_out=None, eos=EOS, child_ptr=p(t.child_ptr),
                child_tok=p(t.child_tok), child_node=p(t.child_node), terminal=p(t.terminal), n_nodes=N, n_edges=E, node_score=p(ns),
                final=p(fin))
    bad = [dict(logits=None), dict(level_node=None), dict(child_ptr=None), dict(terminal=None), dict(node_score=None), dict(final=None),
           dict(child_tok=None), dict(child_node=None), dict(ld=V - 1), dict(V=0), dict(eos=V), dict(eos=-1), dict(b=0), dict(b=-3),
           dict(rows=-6), dict(rows=2 * b + 1), dict(rows=(N + 1) * b), dict(n_nodes=0), dict(n_nodes=1), dict(n_edges=-1)]
    for change in bad:
        with pytest.raises(lib.ValorHipError):
            lib.call("valor_trie_score_level", K._stream(), *dict(good, **change).values())
    torch.cuda.synchronize()
    assert torch.isnan(ns).all() and torch.isnan(fin).all()                         # nothing ran
    lib.call("valor_trie_score_level", K._stream(), *dict(good, rows=0).values())   # no rows: a no-op
    torch.cuda.synchronize()
    assert torch.isnan(ns).all() and torch.isnan(fin).all()


# ------------------------------------------------------------------------------------------------ the small synthetic model
def _model(dev, dtype=torch.float32, **opts):
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=5, w_std=0.05)
    m = VALOR({"dropout": 0.0, "drop_path_rate": 0.0, "max_generation_len": 10, **opts}, spec=spec, dtype=dtype, device=dev)
    m.load_state_dict(sd, strict=True)
    return m, spec


def _batch(spec, b=3, seed=6):
    from valor_amd import synth
    batch = synth.make_batch(spec, batch=b, frames=2, audio_slices=2, txt_len=16, seed=seed, questions=True)
    assert (batch["question_tokens"]["bert_tokens"] == 0).any()                             # zero-padded questions
    batch["ids"] = [f"clip{i}" for i in range(b)]
    return batch


def model_sets(spec):
    """the shared set of tests/test_answer_set_decode_gpu.py (answers of 1..4 tokens with common prefixes), and a second one whose root
    has 300 children"""
    from valor_amd import decode
    g = torch.Generator().manual_seed(11)
    w = torch.randint(200, spec.vocab, (40,), generator=g).tolist()
    shared = decode.AnswerSet([[w[0]], [w[0], w[1]], [w[0], w[1], w[2], w[3]], [w[4], w[5]], [w[6], w[7], w[8]], [w[9]], [w[4], w[10]]])
    firsts = list(range(300, 600))
    wide = decode.AnswerSet([[t] for t in firsts] + [[300, w[1]], [300, w[1], w[2]], [301, w[3], w[4], w[5]]])
    assert wide.levels().width == 300
    return shared, wide


def reference_scores(m, batch, group, a, prompt):
    """teacher-forced on the re-run path: decode.stepper(...).logits, log-softmax and the sum in fp64 -> ([b, C] fp64, lengths [C]). The
    law of reference_scores in tests/test_answer_set_decode_gpu.py; every distinct prefix of a length runs once, as one beam-major
    batch (row = prefix * b + sample)."""
    from valor_amd import decode
    cands = a.candidates[0]
    with torch.no_grad():
        m.eval()
        b, kv_layers, ranges = decode.encode_for_generation(m, batch, [group])
        if torch.is_tensor(prompt):
            assert prompt.shape[0] == b
        step = decode.stepper(m, group, b, kv_layers, ranges, prompt)
        lp = {(): torch.log_softmax(step.logits(None, b).double().cpu(), 1)}
        for t in range(1, a.max_len + 1):
            pres = sorted({tuple(c[:t]) for c in cands if len(c) >= t})
            for p0 in range(0, len(pres), 128):
                part = pres[p0:p0 + 128]
                state = torch.tensor(part, dtype=torch.long)[:, None, :].expand(len(part), b, t).reshape(len(part) * b, t)
                out = torch.log_softmax(step.logits(state, len(part) * b).double().cpu(), 1).view(len(part), b, -1)
                lp.update({p: out[i] for i, p in enumerate(part)})
    score = torch.zeros((b, len(cands)), dtype=torch.float64)
    for c, cand in enumerate(cands):
        for t, w in enumerate(cand + [EOS]):
            score[:, c] += lp[tuple(cand[:t])][:, w]
    return score, torch.tensor([len(c) for c in cands])


def _prompt(m, batch):
    return m.qa_prompt(batch["question_tokens"]["bert_tokens"].cpu())


def _check(sc, ref, lens, what):
    assert sc.is_cuda and sc.dtype == torch.float32 and tuple(sc.shape) == tuple(ref.shape)
    assert not torch.isinf(sc).any() and not torch.isnan(sc).any()                 # a shared set: no -inf slot
    err = (sc.cpu().double() - ref).abs()
    band = ((lens + 1).double() * TERM)[None, :]
    print(f"rank_candidates {what}: max |err| {float(err.max()):.2e} (band per term {TERM})")
    assert (err <= band).all(), (what, float((err / band).max()))


def test_rank_candidates_against_the_rerun_path(dev):
    from valor_amd import decode
    m, spec = _model(dev)
    qb = _batch(spec)
    shared, wide = model_sets(spec)
    prompt = _prompt(m, qb)
    for a, name in ((shared, "shared"), (wide, "wide")):
        m.train()
        got = decode.rank_candidates(m, qb, ["tva", "tv"], a, prompt_cpu=prompt)
        # the session pool is empty after the call and the model's mode is back
        assert set(got) == {"tva", "tv"} and not m.__dict__.get("_decode_sessions") and m.training
        for g in ("tva", "tv"):
            ref, lens = reference_scores(m, qb, g, a, prompt)
            _check(got[g], ref, lens, f"{name} {g}")
    m.eval()
    got = decode.rank_candidates(m, qb, ["tva"], shared)["tva"]                    # the caption prompt
    assert not m.training and not m.__dict__.get("_decode_sessions")
    ref, lens = reference_scores(m, qb, "tva", shared, "caption")
    _check(got, ref, lens, "shared tva, caption prompt")
    plain = decode.rank_candidates(m, qb, ["tva"], shared.candidates[0])["tva"]   # a plain list of token lists is wrapped
    assert same_bits(plain, got)


def test_chunks_and_sub_batches_stay_within_the_band(dev, monkeypatch):
    """max_rows splits the 300-node level into three chunks, the byte cap splits the three samples into two sub-batches"""
    from valor_amd import decode
    m, spec = _model(dev)
    qb = _batch(spec)
    _, wide = model_sets(spec)
    prompt = _prompt(m, qb)
    whole = decode.rank_candidates(m, qb, ["tva"], wide, prompt_cpu=prompt)["tva"]
    seen = []
    inner = decode._rank_tree

    def spy(model, g, b, kv, ranges, pr, a, max_rows):
        lv = a.levels()
        cn = min(lv.width, max(1, max_rows // b))
        seen.append((b, -(-lv.width // cn)))
        return inner(model, g, b, kv, ranges, pr, a, max_rows)
    monkeypatch.setattr(decode, "_rank_tree", spy)
    lens = torch.tensor([len(c) for c in wide.candidates[0]])
    band = ((lens + 1).float() * TERM)[None, :]
    chunked = decode.rank_candidates(m, qb, ["tva"], wide, prompt_cpu=prompt, max_rows=300)["tva"]
    assert seen == [(3, 3)]                                                         # 100 nodes x 3 samples per pass
    assert ((chunked - whole).abs().cpu() <= band).all()
    del seen[:]
    slot_bytes = spec.layers * 2 * spec.hidden * 4
    P, N = prompt.shape[1], wide.n_nodes
    cap = (2 * (P + N) + 300 * 2) * slot_bytes                                      # two samples' slots fit, three do not
    split = decode.rank_candidates(m, qb, ["tva"], wide, prompt_cpu=prompt, max_store_bytes=cap)["tva"]
    assert seen == [(2, 1), (1, 1)]
    assert ((split - whole).abs().cpu() <= band).all()
    del seen[:]
    both = decode.rank_candidates(m, qb, ["tva"], wide, prompt_cpu=prompt, max_rows=200, max_store_bytes=(2 * (P + N) + 200) * slot_bytes)["tva"]
    assert seen == [(2, 3), (1, 2)]
    assert ((both - whole).abs().cpu() <= band).all()
    ref, rl = reference_scores(m, qb, "tva", wide, prompt)
    _check(both, ref, rl, "wide tva, chunks and sub-batches")


def test_top_1_is_what_an_exhaustive_beam_search_chooses(dev):
    """beam 8 over the shared set of 7 answers (4 first tokens): every answer is searched, so the chosen one's exact score is the row's
    maximum, within the tie band of tests/test_answer_set_decode_gpu.py::test_exhaustive_beam_search_picks_the_best_scored_candidate"""
    from valor_amd import decode
    m, spec = _model(dev)
    shared, _ = model_sets(spec)
    try:
        for seed in (6, 9):
            qb = _batch(spec, seed=seed)
            prompt = _prompt(m, qb)
            out = decode.generate_qa(m, qb, ["tva", "tv"], prompt, beam_size=8, candidates=shared)
            full = decode.rank_candidates(m, qb, ["tva", "tv"], shared, prompt_cpu=prompt)
            top = decode.rank_candidates(m, qb, ["tva", "tv"], shared, prompt_cpu=prompt, k=1)
            for g, key in (("tva", "t_va"), ("tv", "t_v")):
                idx = shared.index_of(out["generated_answers_" + key].cpu())
                assert (idx >= 0).all()
                sc = full[g].cpu()
                val, best = top[g][0].cpu(), top[g][1].cpu()
                assert tuple(best.shape) == (3, 1) and best.dtype == torch.int64
                assert same_bits(val[:, 0], sc.max(1).values) and torch.equal(best[:, 0], sc.argmax(1))
                chosen = sc.gather(1, idx[:, None])[:, 0]
                tie = (shared.max_len + 1) * TERM
                assert (chosen >= val[:, 0] - tie).all(), (g, idx, best, sc)
                far = (sc.max(1, keepdim=True).values - sc > tie).sum(1) == sc.shape[1] - 1      # the best stands alone: the same answer
                assert torch.equal(idx[far], best[far, 0])
    finally:
        decode.release_sessions(m)


def test_top_k_descends_with_duplicates_in_index_order(dev):
    from valor_amd import decode
    m, spec = _model(dev)
    qb = _batch(spec)
    shared, _ = model_sets(spec)
    prompt = _prompt(m, qb)
    twice = decode.AnswerSet(shared.candidates[0] * 2)                              # every answer twice: index c and c + 7
    full = decode.rank_candidates(m, qb, ["tva"], twice, prompt_cpu=prompt)["tva"].cpu()
    assert same_bits(full[:, :7], full[:, 7:])                                      # duplicates carry equal scores
    val, idx = decode.rank_candidates(m, qb, ["tva"], twice, prompt_cpu=prompt, k=3)["tva"]
    val, idx = val.cpu(), idx.cpu()
    assert tuple(val.shape) == tuple(idx.shape) == (3, 3) and val.dtype == torch.float32 and idx.dtype == torch.int64
    assert (val[:, 0] >= val[:, 1]).all() and (val[:, 1] >= val[:, 2]).all()
    order = torch.sort(full, dim=1, descending=True, stable=True)                      # stable: equal scores in index order
    assert torch.equal(idx, order.indices[:, :3]) and same_bits(val, order.values[:, :3])
    assert (idx[:, 1] == idx[:, 0] + 7).all() and same_bits(val[:, 0], val[:, 1])   # the lowest duplicate comes first
    with pytest.raises(ValueError, match="k = 15"):
        decode.rank_candidates(m, qb, ["tva"], twice, prompt_cpu=prompt, k=15)


def _against_score_candidates(m, batch, a, prompt, per_term, what):
    from valor_amd import decode
    try:
        got = decode.rank_candidates(m, batch, ["tva"], a, prompt_cpu=prompt)["tva"].cpu()
        want = decode.score_candidates(m, batch, ["tva"], a, prompt_cpu=prompt)["tva"].cpu()
        assert tuple(got.shape) == tuple(want.shape) and not torch.isinf(got).any() and not torch.isinf(want).any()
        lens = torch.tensor([len(c) for c in a.candidates[0]])
        err = (got - want).abs()
        print(f"rank_candidates against score_candidates, {what}: max |err| {float(err.max()):.2e} (band per term {per_term})")
        assert (err <= ((lens + 1).float() * per_term)[None, :]).all(), what
        assert not m.__dict__.get("_decode_sessions")
        return got
    finally:
        decode.release_sessions(m)


def test_caption_type_lm(dev):
    m, spec = _model(dev, caption_type="lm")
    qb = _batch(spec)
    shared, _ = model_sets(spec)
    _against_score_candidates(m, qb, shared, _prompt(m, qb), TERM, "'lm'")


def test_several_question_rows_per_clip(dev):
    from valor_amd import synth
    m, spec = _model(dev)
    qb = _batch(spec)
    shared, _ = model_sets(spec)
    four = synth.make_batch(spec, batch=4, frames=2, audio_slices=2, txt_len=16, seed=9, questions=True)
    sq = dict(qb, question_tokens=four["question_tokens"], sample_num=[2, 1, 1])
    got = _against_score_candidates(m, sq, shared, _prompt(m, sq), TERM, "sample_num [2, 1, 1]")
    assert got.shape[0] == 4


def test_bf16_within_the_logit_error(dev):
    """bf16, the benchmarked arithmetic: both sides carry the bf16 logit error of a step"""
    from test_finetune_gpu import BF16_LOGIT_BAND
    m, spec = _model(dev, dtype=torch.bfloat16)
    qb = _batch(spec)
    shared, wide = model_sets(spec)
    _against_score_candidates(m, qb, shared, _prompt(m, qb), 2 * BF16_LOGIT_BAND, "bf16 shared")


def test_no_tree_pass_delegates_to_score_candidates(dev, monkeypatch):
    """VALOR_KV_CACHE=0: the same interface over score_candidates"""
    from valor_amd import decode
    m, spec = _model(dev)
    qb = _batch(spec)
    shared, _ = model_sets(spec)
    prompt = _prompt(m, qb)
    monkeypatch.setenv("VALOR_KV_CACHE", "0")
    monkeypatch.setattr(decode, "_rank_tree", None)
    got = decode.rank_candidates(m, qb, ["tva"], shared, prompt_cpu=prompt)["tva"]
    want = decode.score_candidates(m, qb, ["tva"], shared, prompt_cpu=prompt)["tva"]
    assert same_bits(got, want)
    val, idx = decode.rank_candidates(m, qb, ["tva"], shared, prompt_cpu=prompt, k=1)["tva"]
    assert torch.equal(idx[:, 0], want.argmax(1))


# ------------------------------------------------------------------------------------------------ evaluation
RIGHT = [500, 501]


def plant(m):
    """the known answer: the decoder bias makes 500 the likeliest token, then 501, then [SEP]"""
    with torch.no_grad():
        bias = m.P["cls.decoder.bias"]
        bias[500] += 40.0
        bias[501] += 30.0
        bias[EOS] += 20.0


def dec(seqs):
    return [" ".join(str(int(x)) for x in (r[:r.index(EOS)] if EOS in r else r)) for r in seqs.tolist()]


def bert_rows(cands, T=8):
    rows = torch.zeros((len(cands), T), dtype=torch.long)
    for i, c in enumerate(cands):
        rows[i, 0], rows[i, 1:1 + len(c)], rows[i, 1 + len(c)] = 101, torch.tensor(c), EOS
    return rows


def loader_of(spec):
    """two batches of three questions in the training schema ('[CLS] answer [SEP]' rows); the answer is [500 501] for the first batch
    and [600] for the second, so that an accuracy between 0 and 100 is possible"""
    batches = []
    for n, seed in enumerate((6, 9)):
        batch = _batch(spec, seed=seed)
        batch["txt_tokens"] = {"bert_tokens": bert_rows([RIGHT if n == 0 else [600]] * 3)}
        batch["question_ids"] = [f"q{n}_{q}" for q in range(3)]
        batches.append(batch)
    return batches


def test_validate_qa_exact_ranking(dev, tmp_path):
    from valor_amd import decode
    from valor_amd.evaluate import validate_qa
    cands = [[600], [500, 700], RIGHT, [501, 640, 650], RIGHT]
    m, spec = _model(dev)
    mo, _ = _model(dev, qa_answer_candidates=cands, qa_answer_ranking="exact")
    plant(m), plant(mo)
    loader = loader_of(spec)
    try:
        # what the arg max of score_candidates says, question by question (the first column that holds the row maximum)
        want = {"tva": [], "tv": []}
        for batch in loader:
            sc = decode.score_candidates(m, batch, ["tva", "tv"], cands, prompt_cpu=_prompt(m, batch))
            for g in want:
                want[g] += [" ".join(str(w) for w in cands[int(i)]) for i in sc[g].argmax(1).cpu()]
        assert want["tv"] == ["500 501"] * 6                                        # the planted answer wins everywhere: half are right
        gt = ["500 501"] * 3 + ["600"] * 3
        acc = {g: {"accuracy": round(100 * sum(p == t for p, t in zip(want[g], gt)) / 6, 2)} for g in ("tv", "tva")}
        before = validate_qa(m, loader, "qa%tva%tv", decode=dec, candidates=cands, output_dir=str(tmp_path / "a"), global_step=1)
        log = validate_qa(m, loader, "qa%tva%tv", decode=dec, candidates=decode.AnswerSet(cands), answer_ranking="exact",
                          output_dir=str(tmp_path / "b"), global_step=1, dset_name="x")
        assert log == acc == {"tv": {"accuracy": 50.0}, "tva": {"accuracy": 50.0}}
        folder = tmp_path / "b" / "predict_answers"
        assert json.load(open(folder / "step1_gt.json")) == gt
        assert json.load(open(folder / "step1_tv_pred.json")) == want["tv"]
        sub = json.load(open(folder / "step1_tv_pred_submited_x.json"))
        assert [r["question_id"] for r in sub] == [f"q{n}_{q}" for n in range(2) for q in range(3)] and [r["answer"] for r in sub] == want["tv"]
        assert validate_qa(mo, loader, "qa%tv", decode=dec) == {"tv": acc["tv"]}    # the options are the defaults
        # the default ranking is the constrained decode, untouched: the same log and the same files as 'decode' named aloud
        again = validate_qa(m, loader, "qa%tva%tv", decode=dec, candidates=cands, answer_ranking="decode", output_dir=str(tmp_path / "c"),
                            global_step=1)
        assert before == again
        for name in ("step1_gt.json", "step1_tv_pred.json", "step1_tv_pred_submited_.json"):
            assert json.load(open(tmp_path / "a" / "predict_answers" / name)) == json.load(open(tmp_path / "c" / "predict_answers" / name))
    finally:
        decode.release_sessions(m)
        decode.release_sessions(mo)
