"""Model-level data-parallel correctness on the GPU: 2 processes share cuda:0 (gloo: RCCL refuses two ranks on one device; the
collectives' SEMANTICS are what is under test, the transport is covered by bench.py --gpus N over nccl), each runs the native fp32
model on its half of a batch through TrainEngine (packed feature all-gather with local-slice backward, gradient reducer on the
flat arena, fused optimizer). Expectations come from the CPU oracle with the reference's gather semantics restated
(utils/distributed.py:38-93: every rank computes the contrastive loss on the GLOBAL batch, backward keeps the local slice only;
DDP then averages the gradients -- so the contrastive gradient is 1/world of the single-process one, the reference's quirk):
  * contra_loss is identical on both ranks and equals the single-process loss on the full batch;
  * caption / mlm losses are each rank's own;
  * the reduced gradient (arena sum / world) equals the mean over ranks of the oracle's per-rank gradients, and for parameters
    that only feed the contrastive loss it is 1/world of the single-process full-batch gradient;
  * after an optimizer step (overlapped bucket path on the second step) the replicas hold identical parameters."""
import os
import random
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TASK = "pt_contra%tva%tv%ta_caption%tva%tv%ta_mlm%tva"
B_LOCAL, FRAMES, SLICES = 2, 2, 1
RANKS_PER_GPU = 4          # rank processes sharing one device at most (rank r runs on GPU r % device_count; the test process holds GPU 0 too)


def _skip_unless_gpus_for(world):
    """decided before any work: `world` ranks at RANKS_PER_GPU per device need this many GPUs"""
    need, have = -(-world // RANKS_PER_GPU), torch.cuda.device_count()
    if have < need:
        pytest.skip(f"{world} ranks need {need} GPUs ({RANKS_PER_GPU} ranks per GPU), found {have}")


def _setup(world=2):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from valor_amd import synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    full = synth.make_batch(spec, batch=world * B_LOCAL, frames=FRAMES, audio_slices=SLICES, txt_len=32, seed=4)
    return spec, sd, full


def _half(full, r):
    sl = slice(r * B_LOCAL, (r + 1) * B_LOCAL)
    return {"ids": full["ids"][sl], "video_pixels": full["video_pixels"][sl], "audio_spectrograms": full["audio_spectrograms"][sl],
            "txt_tokens": {k: v[sl] for k, v in full["txt_tokens"].items()}}


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from types import SimpleNamespace
        spec, sd, full = _setup(world)
        from valor_amd.engine import TrainEngine
        from valor_amd.model.valor import VALOR
        device = torch.device("cuda", rank % torch.cuda.device_count())
        torch.cuda.set_device(device)
        model = VALOR({"dropout": 0.0}, spec=spec, dtype=torch.float32, device=device)
        if rank == 0:
            model.load_state_dict(sd, strict=True)          # rank 1 starts from zeros: TrainEngine's broadcast must fix that
        opts = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-3, clip_lr_text=1e-3, new_lr=0.0, decoder_lr=-1,
                               betas=[0.9, 0.98], warmup_ratio=0.1, num_train_steps=10, scheduler="warmup_linear", grad_norm=5.0)
        eng = TrainEngine(model, opts, manage_gc=False)
        assert eng.world == world and model.gather_fn is not None
        batch = _half(full, rank)
        model.train()
        random.seed(100 + rank)
        eng.reducer.prepare_backward()
        out = model(batch, task=TASK, compute_loss=True)
        sum(out.values()).backward()
        eng.reducer.finish_backward()
        torch.cuda.synchronize()
        grads = {}
        for name, shape, refs in model.table:
            g = model.P[name].grad.detach().cpu().clone()
            if len(refs) == 1 or refs[1] == "cls.decoder.weight":
                grads[refs[0]] = g
            else:
                rows = shape[0] // len(refs)
                for i, r in enumerate(refs):
                    grads[r] = g[i * rows:(i + 1) * rows]
        model.arena.grad.zero_()
        # two real optimizer steps (first: synchronous learn-the-used-set path, second: overlapped buckets)
        for step in range(2):
            random.seed(200 + 10 * step + rank)
            eng.train_step(batch, TASK)
        torch.cuda.synchronize()
        torch.save({"losses": {k: float(v) for k, v in out.items()}, "grads": grads, "flat": model.arena.flat.detach().cpu().clone()},
                   os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("W", [2, 4, 8])
def test_ranks_match_the_reference_semantics(dev, tmp_path, W):
    """world 2 / 4 / 8 (every rank a process, RANKS_PER_GPU of them per GPU, gloo): nothing above world 2 had ever executed before round 4"""
    _skip_unless_gpus_for(W)
    spec, sd, full = _setup(W)
    import valor_oracle as VO
    from valor_amd import synth
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(W, port, str(tmp_path)), nprocs=W, join=True)
    res = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"), weights_only=False) for r in range(W)]

    vocab = synth.synthetic_vocab(spec.vocab)
    # features every rank contributes to the gather (constants for the OTHER rank's backward)
    feats = []
    with torch.no_grad():
        for r in range(W):
            orc = VO.Oracle(spec, sd, vocab_tokens=vocab)
            ev = orc.forward_pt(_half(full, r), "pt_contra%tva%tv%ta", compute_loss=False)
            feats.append({k: ev[k] for k in ("feat_t", "feat_v", "feat_a", "txt_tokens")})
    want_grads, want_losses = [], []
    for r in range(W):
        sd_r = VO.trainable_copy(sd)
        orc = VO.Oracle(spec, sd_r, vocab_tokens=vocab)

        def gather_feat(f, r=r):
            key = {32: "feat_t", FRAMES: "feat_v", SLICES: "feat_a"}[f.shape[1]]
            parts = [feats[q][key] for q in range(W)]
            parts[r] = f                                             # the local slice carries the gradient (utils/distributed.py:62-72)
            return torch.cat(parts, dim=0)

        def gather_tok(t, r=r):
            return torch.cat([feats[q]["txt_tokens"] for q in range(W)], dim=0)

        random.seed(100 + r)
        out = orc.forward_pt(_half(full, r), TASK, compute_loss=True, gather=(gather_feat, gather_tok))
        sum(out.values()).backward()
        want_losses.append({k: float(v) for k, v in out.items()})
        want_grads.append({k: (p.grad.clone() if p.grad is not None else None) for k, p in sd_r.items()
                           if p.is_floating_point() and not VO.is_alias_key(k)})
    # single process on the full batch: the contrastive loss (masker-independent) and its gradients
    sd_f = VO.trainable_copy(sd)
    lf = VO.Oracle(spec, sd_f, vocab_tokens=vocab).forward_pt(full, "pt_contra%tva%tv%ta", compute_loss=True)["contra_loss"]
    lf.backward()
    full_contra = float(lf)

    for r in range(W):
        for k, v in want_losses[r].items():
            assert abs(res[r]["losses"][k] - v) <= 1e-4 * abs(v), (r, k, res[r]["losses"][k], v)
        assert abs(res[r]["losses"]["contra_loss"] - full_contra) <= 1e-4 * abs(full_contra)
        assert res[0]["losses"]["contra_loss"] == pytest.approx(res[r]["losses"]["contra_loss"], rel=1e-6)
    # the reducer leaves the SUM over ranks in both arenas; DDP's mean is folded into the optimizer
    bad = []
    for k in want_grads[0]:
        parts = [g[k] for g in want_grads if g[k] is not None]
        for r in range(W):
            got = res[r]["grads"][k].double() / W
            if not parts:
                assert float(got.abs().max()) == 0.0, k
                continue
            want = sum(p.double() for p in parts) / W
            scale = max(float(want.norm()), 1e-5 * want.numel() ** 0.5)
            err = float((got.reshape(want.shape) - want).norm()) / scale
            if err > 2e-3:
                bad.append((r, k, err))
    assert not bad, bad[:8]
    # the reference's quirk, stated directly: the CLIP text tower only feeds the contrastive loss, each rank back-propagates the
    # local slice of the gathered-feature gradient, DDP averages -> 1/world of the single-process full-batch gradient
    for k in ("clip_model.text_projection", "clip_model.transformer.resblocks.0.attn.in_proj_weight", "clip_model.token_embedding.weight"):
        got = res[0]["grads"][k].double() / W
        want = sd_f[k].grad.double() / W
        assert float((got.reshape(want.shape) - want).norm()) <= 2e-3 * float(want.norm()), k
    # ... while parameters applied to the GATHERED features (fine-weight heads, temperature) see the full gradient on every rank
    for k in ("text_fine_weight.0.weight", "clip_model.logit_scale"):
        got = res[0]["grads"][k].double() / W
        want = sd_f[k].grad.double()
        assert float((got.reshape(want.shape) - want).norm()) <= 2e-3 * float(want.norm()) + 1e-9, k
    for r in range(1, W):
        assert torch.equal(res[0]["flat"], res[r]["flat"]), "replicas diverged after two optimizer steps"
    assert float(res[0]["flat"].abs().sum()) > 0


def _graph_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from types import SimpleNamespace
        spec, sd, full = _setup(world)
        from valor_amd import ops
        from valor_amd.engine import TrainEngine
        from valor_amd.model.valor import VALOR
        torch.cuda.set_device(0)
        res = {}
        for graphs in (False, True):
            model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device="cuda:0")
            model.load_state_dict(sd, strict=True)
            opts = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-3, clip_lr_text=1e-3, new_lr=0.0, decoder_lr=-1,
                                   betas=[0.9, 0.98], warmup_ratio=0.1, num_train_steps=10, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0)
            eng = TrainEngine(model, opts, manage_gc=False, graphs=graphs)
            eng.optimizer.init_master_from(sd)
            if not graphs:
                ops.DropoutState.enable_device_base(torch.device("cuda:0"))
            ops.DropoutState.reset(7 + rank)
            batch = _half(full, rank)
            batch["video_pixels"] = batch["video_pixels"].cuda()
            batch["audio_spectrograms"] = batch["audio_spectrograms"].cuda()
            random.seed(300 + rank)
            losses = []
            for step in range(5):                       # steps 0-1 eager (the used-parameter set is learnt on 0), capture inside step 2, replays from then on
                out = eng.train_step(batch, TASK)
                losses.append({k: float(v) for k, v in out.items()})
            torch.cuda.synchronize()
            res[graphs] = {"losses": losses, "flat": model.arena.flat.detach().cpu().clone(),
                           "captured": sorted(model._graph_segs) if graphs else []}
            model.enable_graphs(False)
            eng.close()
            ops.DropoutState.disable_device_base()
            del model, eng
        torch.save(res, os.path.join(outdir, f"graph_rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_graphed_encoders_in_data_parallel(dev, tmp_path):
    """hipGraph replay of the encoders under data parallelism (world 2, gloo on the one GPU, dropout 0.1, bf16): the reducer's bookkeeping is
    replayed from the capture-time schedule, buckets leave while the rest of the backward is still being issued. Five optimizer steps with
    the graphs against five eager steps of the same seeds: bit-identical losses on every rank and step, bit-identical parameters, and the
    replicas identical to each other."""
    import socket
    W = 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_graph_worker, args=(W, port, str(tmp_path)), nprocs=W, join=True)
    res = [torch.load(os.path.join(str(tmp_path), f"graph_rank{r}.pt"), weights_only=False) for r in range(W)]
    for r in range(W):
        assert res[r][True]["captured"] == ["ast", "clip_text", "decoder", "vit"]
        assert res[r][True]["losses"] == res[r][False]["losses"], (r, res[r][True]["losses"], res[r][False]["losses"])
        assert torch.equal(res[r][True]["flat"], res[r][False]["flat"])
    assert torch.equal(res[0][True]["flat"], res[1][True]["flat"]), "replicas diverged"
    assert res[0][True]["losses"][0]["contra_loss"] == res[1][True]["losses"][0]["contra_loss"]     # the gathered contrastive loss is global


def _nccl_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda:0"))
    try:
        from valor_amd.arena import ParamArena
        from valor_amd.dist import Reducer, _PackedGather
        arena = ParamArena([(f"p{i}", (5000 + 8 * i,), 0) for i in range(6)], torch.bfloat16, "cuda:0")
        res = {}
        for mode in ("allreduce", "rs_ag", "fp32"):
            red = Reducer(arena, bucket_bytes=16384, mode=mode)
            g = torch.Generator().manual_seed(3)
            want = torch.randn(arena.numel, generator=g).bfloat16().cuda()
            arena.grad.copy_(want)
            for w in red._reduce(arena.grad):                 # the collectives themselves, over RCCL (world 1: the sum is the input)
                w.wait()
            torch.cuda.synchronize()
            res[mode] = bool(torch.equal(arena.grad, want))
        ft = torch.randn(3, 4, 8, device="cuda:0").bfloat16()
        out = _PackedGather.apply(ft, ft[:, :2])
        torch.cuda.synchronize()
        res["gather"] = bool(torch.equal(out[0], ft) and torch.equal(out[1], ft[:, :2]))
        torch.save(res, os.path.join(outdir, "nccl.pt"))
    finally:
        dist.destroy_process_group()


def test_rccl_collectives_execute(dev, tmp_path):
    """the collectives of valor_amd.dist over the nccl backend (= RCCL) on the GPU box: one rank is all a 1-GPU box offers, but
    all_reduce / reduce_scatter_tensor + all_gather_into_tensor / the packed feature gather all go through RCCL's kernels and
    must hand back the input unchanged (bench.py --gpus N runs the same calls with N ranks)."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_nccl_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    res = torch.load(os.path.join(str(tmp_path), "nccl.pt"))
    assert res == {"allreduce": True, "rs_ag": True, "fp32": True, "gather": True}, res


def test_bench_gpus_flag_launches_that_many_ranks():
    """`python bench.py --gpus 2` started WITHOUT a launcher must really run two ranks (it re-executes itself under
    torch.distributed.run) and say so in its JSON line; the two ranks share this box's one GPU over gloo (RCCL refuses duplicate devices;
    on a multi-GPU node the same command runs one rank per GPU over RCCL). Replaces the DDP launch of scripts/pretrain.sh:3
    (python -m torch.distributed.launch --nproc_per_node 8) for the bench."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["VALOR_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--batch", "4", "--steps", "2", "--warmup", "1",
                        "--frames", "2", "--audio-slices", "1", "--no-cpu-baseline", "--no-roofline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2 and res["ranks"] == 2 and res["backend"] == "gloo"
    assert res["config"]["global_batch"] == 8 and res["config"]["parallelism"] == "dp2"
    assert all(v == v and abs(v) < 1e4 for v in res["losses"].values())
    assert res["replicas_identical"] is True


def test_bench_with_eight_ranks_on_one_gpu():
    """the driver's 8-GPU command line (`bench.py --gpus 8`) with the eight ranks sharing the node's GPUs over gloo (bench.py puts rank r
    on GPU r % device_count, RANKS_PER_GPU per device at most), at a batch that fits eight replicas: eight ranks really run, the losses
    are finite and every replica holds bit-identical parameters after the timed steps (the line's `replicas_identical` = an
    all-gathered checksum of the parameter arena)"""
    _skip_unless_gpus_for(8)
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["VALOR_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--batch", "2", "--steps", "2", "--warmup", "1",
                        "--frames", "2", "--audio-slices", "1", "--no-cpu-baseline", "--no-roofline"], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["n_gpus"] == 8 and res["ranks"] == 8 and res["backend"] == "gloo"
    assert res["config"]["global_batch"] == 16 and res["config"]["parallelism"] == "dp8"
    assert all(v == v and abs(v) < 1e4 for v in res["losses"].values())
    assert res["replicas_identical"] is True


def _eval_shards():
    """three validation batches, the last one smaller: rank 0 scores batches 0 and 2 (4 + 2 samples), rank 1 batch 1 (4 samples)"""
    sys.path.insert(0, ROOT)
    from valor_amd import synth
    spec = synth.tiny_spec()
    sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
    bs = []
    for i, n in enumerate((4, 4, 2)):
        b = synth.make_batch(spec, batch=n, frames=2, audio_slices=1, txt_len=32, seed=10 + i)
        b["ids"] = [f"v{10 * i + j}" for j in range(n)]
        b["ids_txt"] = list(b["ids"])
        bs.append(b)
    return spec, sd, [[bs[0], bs[2]], [bs[1]]]


def _eval_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        spec, sd, shards = _eval_shards()
        from valor_amd.evaluate import validate_pt
        from valor_amd.model.valor import VALOR
        torch.cuda.set_device(0)
        model = VALOR({"dropout": 0.0}, spec=spec, dtype=torch.float32, device="cuda:0")
        model.load_state_dict(sd, strict=True)
        random.seed(50 + rank)
        log = validate_pt(model, shards[rank], TASK)
        torch.save(log, os.path.join(outdir, f"eval{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_validate_pt_gathers_the_ranks_shards(tmp_path):
    """validate_pt under two ranks with UNEQUAL shards (6 and 4 samples) returns on every rank what one process returns for the ten
    samples: ids and hit counters through all_gather_list, features / tokens through ddp_allgather (test.py:275-290, 496-518;
    utils/distributed.py:77-93). The single process walks the shards in rank order with the ranks' masker seeds."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_eval_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    logs = [torch.load(tmp_path / f"eval{r}.pt", weights_only=False) for r in range(2)]
    spec, sd, shards = _eval_shards()
    from valor_amd.evaluate import validate_pt
    from valor_amd.model.valor import VALOR
    model = VALOR({"dropout": 0.0}, spec=spec, dtype=torch.float32, device="cuda:0")
    model.load_state_dict(sd, strict=True)

    def walk():
        for r, shard in enumerate(shards):
            random.seed(50 + r)
            yield from shard
    one = validate_pt(model, walk(), TASK)
    assert {"caption_acc_tva", "mlm_acc_tva", "t2v_recall", "t2va_recall", "t2a_recall"} <= set(one)
    assert logs[0] == one and logs[1] == one, (logs, one)


def _nccl_graph_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda:0"))
    try:
        from types import SimpleNamespace
        from valor_amd import ops, synth
        from valor_amd.engine import TrainEngine
        from valor_amd.model.valor import VALOR
        spec = synth.tiny_spec()
        sd = synth.make_state_dict(spec, seed=3, w_std=0.05)
        batch = synth.make_batch(spec, batch=4, frames=2, audio_slices=1, txt_len=32, seed=4)
        batch["video_pixels"] = batch["video_pixels"].cuda()
        batch["audio_spectrograms"] = batch["audio_spectrograms"].cuda()
        res = {}
        side = torch.cuda.Stream()
        x = torch.ones(1 << 20, device="cuda:0")
        for graphs in (False, True):
            model = VALOR({"dropout": 0.1}, spec=spec, dtype=torch.bfloat16, device="cuda:0")
            model.load_state_dict(sd, strict=True)
            opts = SimpleNamespace(learning_rate=1e-3, weight_decay=0.01, clip_lr=1e-3, clip_lr_text=1e-3, new_lr=0.0, decoder_lr=-1,
                                   betas=[0.9, 0.98], warmup_ratio=0.1, num_train_steps=10, scheduler="warmup_linear", grad_norm=5.0, alloc_headroom_mb=0)
            eng = TrainEngine(model, opts, manage_gc=False, graphs=graphs)
            eng.optimizer.init_master_from(sd)
            if not graphs:
                ops.DropoutState.enable_device_base(torch.device("cuda:0"))
            ops.DropoutState.reset(11)
            random.seed(400)
            losses = []
            for step in range(5):
                with torch.cuda.stream(side):          # RCCL work in flight (and its watchdog polling it) while step 2 captures its graphs
                    works = [dist.all_reduce(x, async_op=True) for _ in range(4)]
                out = eng.train_step(batch, TASK)
                for w in works:
                    w.wait()
                losses.append({k: float(v) for k, v in out.items()})
            torch.cuda.synchronize()
            res[graphs] = {"losses": losses, "flat": model.arena.flat.detach().cpu().clone(), "captured": sorted(model._graph_segs)}
            model.enable_graphs(False)
            eng.close()
            ops.DropoutState.disable_device_base()
            del model, eng
        torch.save(res, os.path.join(outdir, "nccl_graph.pt"))
    finally:
        dist.destroy_process_group()


def test_graph_capture_with_an_rccl_process_group_up(dev, tmp_path):
    """capture inside a training step while an RCCL (nccl backend) process group exists and has collectives in flight: ProcessGroupNCCL's
    watchdog thread polls their events from another thread, which a capture in the default "global" error mode may take for a violation
    (the documented DDP + CUDA graphs caveat) -- graphs.py captures in "thread_local" mode once a process group is up. Five steps with
    the graphs equal five eager steps to the bit."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_nccl_graph_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    res = torch.load(os.path.join(str(tmp_path), "nccl_graph.pt"), weights_only=False)
    assert res[True]["captured"] == ["ast", "clip_text", "decoder", "vit"]
    assert res[True]["losses"] == res[False]["losses"]
    assert torch.equal(res[True]["flat"], res[False]["flat"])
