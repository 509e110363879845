"""Checkpoint interop of the reference's loading paths (host side, load time only; torch CPU ops are fine here):

  * adapt_pretrained_checkpoint: what train_utils.py::load_from_pretrained_dir does to a `model_step_N.pt` before
    VALOR.from_pretrained sees it (train_utils.py:146-168): frame embeddings beyond the pretraining sample count repeat the last
    trained frame, CLIP's visual positional embedding is bilinearly resized when the video resolution changes; the model options
    the pretraining run fixed are copied over the current ones (:134-144).
  * resize_clip_positional_embedding: the same resize for a bare `--checkpoint` (train.py:28-44).
  * the component checkpoints the reference's constructor reads from ./pretrained_weights (the first pretraining run starts from
    them, train.py:17,55 with checkpoint = {}): AST (modeling.py:512-554, incl. the bilinear resize of its positional embedding
    :520-528), CLIP (:560-573 + clip.py:470-515), VideoSwin (:591-600) and BERT + prediction head (:613-660) key mappings into
    VALOR state-dict keys -- load_pretrained_components() merges them into ONE dict for VALOR.from_pretrained(opts, dict).
The optimizer side (`optimizer_step_N.pt`, --resume) is FusedAdamW.load_reference_state_dict / reference_state_dict.

  * save_run / latest_step / resume_run: exact-resume checkpoints of a training run in the reference's layout (utils/save.py:38-64,
    train_utils.py:174-192) plus one engine file per rank -- see the section at the end of this file.
"""
import os
import re
import threading
import time

import torch
import torch.nn.functional as F

# train_utils.py:134-141
COVER_CFG = ["audio_melbins", "audio_patch_size", "audio_mean", "audio_std", "audio_frame_shift", "audio_target_length",
             "video_encoder_type", "txt_encoder_type", "multimodal_encoder_type", "audio_encoder_type", "caption_type",
             "share_txt_and_multimodal", "contra_type", "multimodal_use_cross_attn", "fineweight_type", "has_vafusion_encoder",
             "late_fusion", "cross_attn_type", "task_pormpt_as_text", "use_task_prompt"]


def resize_clip_positional_embedding(checkpoint, video_resolution):
    """train_utils.py:153-168 / train.py:28-44: keep the cls row, resize the grid rows with F.interpolate(mode='bilinear')."""
    key = "clip_model.visual.positional_embedding"
    if key not in checkpoint:
        return checkpoint
    src = checkpoint[key]
    width = checkpoint["clip_model.visual.conv1.weight"].shape[0]
    patch = checkpoint["clip_model.visual.conv1.weight"].shape[-1]
    grid = round((src.shape[0] - 1) ** 0.5)
    new_grid = video_resolution // patch
    oth = src[1:].reshape(grid, grid, width).permute(2, 0, 1).unsqueeze(0)
    oth = F.interpolate(oth, (new_grid, new_grid), mode="bilinear")
    oth = oth[0].permute(1, 2, 0).reshape(-1, src.shape[-1])
    checkpoint[key] = torch.cat((src[0:1], oth), dim=0)
    return checkpoint


def adapt_pretrained_checkpoint(checkpoint, pretrain_cfg, opts):
    """checkpoint: reference-keyed state dict (a `module.` prefix is stripped); pretrain_cfg: the run's log/hps.json as a dict;
    opts: the current options (namespace or dict), updated in place like train_utils.py:142-144. Returns the adapted dict."""
    checkpoint = {k.replace("module.", ""): v for k, v in checkpoint.items()}
    get = (lambda k, d=None: opts.get(k, d)) if isinstance(opts, dict) else (lambda k, d=None: getattr(opts, k, d))
    for k in COVER_CFG:
        if k in pretrain_cfg:
            if isinstance(opts, dict):
                opts[k] = pretrain_cfg[k]
            else:
                setattr(opts, k, pretrain_cfg[k])
    if "video_frame_embedding" in checkpoint:
        n = pretrain_cfg["video_sample_num"]
        checkpoint["video_frame_embedding"][:, n:] = checkpoint["video_frame_embedding"][:, n - 1].clone()
    if "audio_frame_embedding" in checkpoint:
        n = pretrain_cfg["audio_sample_num"]
        checkpoint["audio_frame_embedding"][:, n:] = checkpoint["audio_frame_embedding"][:, n - 1].clone()
    if get("video_resolution") != pretrain_cfg["video_resolution"] and str(get("video_encoder_type", "")).startswith("clip"):
        resize_clip_positional_embedding(checkpoint, get("video_resolution"))
    return checkpoint


# ------------------------------------------------------------------------------------------ component checkpoints
def ast_to_valor(ast_weight, audio_melbins=64, audio_target_length=512, audio_patch_size=16):
    """initialize_audio_weights, modeling.py:512-554: the AudioSet AST checkpoint (timm DeiT keys under `module.v.`) -> VALOR keys.
    The packed qkv rows are split into linears.0/1/2, the distillation token is dropped, and the positional embedding (cls + 12 x 101
    patches of the 128-mel / 1024-frame pretraining geometry) is resized bilinearly to (melbins / patch) x (target_length / patch)."""
    W = ast_weight["module.v.cls_token"].shape[-1]
    out = {"audio_embeddings.cls_token": ast_weight["module.v.cls_token"],
           "audio_embeddings.first_conv.weight": ast_weight["module.v.patch_embed.proj.weight"],
           "audio_embeddings.first_conv.bias": ast_weight["module.v.patch_embed.proj.bias"]}
    pos = ast_weight["module.v.pos_embed"][0]
    oth = pos[2:].reshape(12, 101, -1).permute(2, 0, 1).unsqueeze(0)                  # [1, W, 12, 101]; row 1 is the distilled token
    th, tw = audio_melbins // audio_patch_size, audio_target_length // audio_patch_size
    oth = F.interpolate(oth, size=(th, tw), mode="bilinear").squeeze().permute(1, 2, 0).reshape(-1, W)
    out["audio_embeddings.position_embeddings.weight"] = torch.cat((pos[0:1], oth), dim=0)
    nl = len({k.split(".")[3] for k in ast_weight if k.startswith("module.v.blocks.")})
    for i in range(nl):
        s, d = f"module.v.blocks.{i}.", f"audio_encoder.layer.{i}."
        for j in range(3):
            out[d + f"attention.linears.{j}.weight"] = ast_weight[s + "attn.qkv.weight"][j * W:(j + 1) * W, :]
            out[d + f"attention.linears.{j}.bias"] = ast_weight[s + "attn.qkv.bias"][j * W:(j + 1) * W]
        out[d + "attention.linears.3.weight"] = ast_weight[s + "attn.proj.weight"]
        out[d + "attention.linears.3.bias"] = ast_weight[s + "attn.proj.bias"]
        for a, b in (("ff_layer.linear1", "mlp.fc1"), ("ff_layer.linear2", "mlp.fc2"), ("layernorm1", "norm1"), ("layernorm2", "norm2")):
            out[d + a + ".weight"] = ast_weight[s + b + ".weight"]
            out[d + a + ".bias"] = ast_weight[s + b + ".bias"]
    out["audio_encoder.last_layernorm.weight"] = ast_weight["module.v.norm.weight"]
    out["audio_encoder.last_layernorm.bias"] = ast_weight["module.v.norm.bias"]
    return out


def clip_to_valor(clip_sd, video_resolution):
    """load_clip_model + build_model, modeling.py:560-573 / clip.py:470-515: OpenAI CLIP state dict -> `clip_model.` keys in fp32, the
    visual positional embedding resized to video_resolution when it differs from the checkpoint's native grid (clip.py:481-491)."""
    # build_model resizes FIRST (on the checkpoint's own dtype), then loads into a model whose Conv / Linear / MultiheadAttention
    # tensors and projections were converted to fp16 (clip.py:446-467 convert_weights, :516-520), then .float() (modeling.py:573):
    # those tensors are fp16-representable in the reference (a no-op for the released fp16 checkpoints)
    out = {"clip_model." + k: v for k, v in clip_sd.items() if k not in ("input_resolution", "context_length", "vocab_size")}
    out = resize_clip_positional_embedding(out, video_resolution)
    half = lambda k: (k.endswith(("conv1.weight", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "c_fc.weight",
                                  "c_fc.bias", "c_proj.weight", "c_proj.bias")) or k in ("clip_model.text_projection", "clip_model.visual.proj"))
    return {k: (v.half().float() if half(k) else v.float()) for k, v in out.items()}


def swin_to_valor(swin_sd):
    """load_videoswin_model, modeling.py:591-600: SwinTransformer3D state dict -> `video_encoder.` keys (the integer
    relative_position_index buffers ride along; VALOR.load_state_dict regenerates and ignores them)."""
    return {"video_encoder." + k: v for k, v in swin_sd.items()}


def bert_to_valor(bert_weight, share_txt_and_multimodal=True):
    """load_bert_model, modeling.py:613-660: HF bert-base-uncased.bin -> `multimodal_encoder.` keys (`bert.` prefix stripped, the old
    gamma / beta LayerNorm names renamed, strict=False: the cross-attention blocks and the prompt embedding keep their
    initialisation) + the prediction head (`cls.predictions.*` -> cls.dense / cls.layernorm / cls.decoder.bias; the decoder
    weight is tied to the word embeddings, modeling.py:241)."""
    ren = {k.replace("bert.", "").replace("gamma", "weight").replace("beta", "bias"): v for k, v in bert_weight.items()}
    out = {"multimodal_encoder." + k: v for k, v in ren.items() if not k.startswith("cls.")}
    head = {"cls.dense.weight": "cls.predictions.transform.dense.weight", "cls.dense.bias": "cls.predictions.transform.dense.bias",
            "cls.layernorm.weight": "cls.predictions.transform.LayerNorm.weight", "cls.layernorm.bias": "cls.predictions.transform.LayerNorm.bias",
            "cls.decoder.bias": "cls.predictions.bias"}
    for dst, src in head.items():
        out[dst] = ren[src]
    # cls.decoder.weight: the reference loads it INTO the tied word-embedding tensor (cls.load_state_dict, modeling.py:650-653)
    out["multimodal_encoder.embeddings.word_embeddings.weight"] = ren["cls.predictions.decoder.weight"]
    return out


PRETRAINED_FILES = {   # modeling.py:514, 563-570, 592-599, 622
    "ast": "audioset_10_10_0.4593.pth", "bert_base_uncased": "bert-base-uncased.bin",
    "clip_vit_base_16": "clip-vit-base-16.pt", "clip_vit_base_32": "clip-vit-base-32.pt", "clip_vit_large_14": "clip-vit-large-14.pt",
    "clip_vit_large_14_336px": "clip-vit-large-14-336px.pt", "videoswin_small_k400_1k": "ckpt_video-swin.pt",
    "videoswin_base_k400_1k": "videoswin_base_k400_1k.pth", "videoswin_base_k400_22k": "videoswin_base_k400_22k.pth",
    "videoswin_base_k600_22k": "videoswin_base_k600_22k.pth",
}


def load_pretrained_components(opts, root="./pretrained_weights", load=None, jit_load=None):
    """What the reference's constructor pulls from ./pretrained_weights for `opts` (modeling.py:296-330), as ONE VALOR-keyed state dict
    for VALOR.from_pretrained(opts, sd): the component checkpoints named by video_encoder_type / txt_encoder_type /
    audio_encoder_type / multimodal_encoder_type. `load` / `jit_load` default to torch.load / torch.jit.load(...).state_dict()."""
    get = (lambda k, d=None: opts.get(k, d)) if isinstance(opts, dict) else (lambda k, d=None: getattr(opts, k, d))
    load = load or (lambda p: torch.load(p, map_location="cpu"))
    jit_load = jit_load or (lambda p: torch.jit.load(p, map_location="cpu").state_dict())
    sd = {}
    clip_type = None
    for t in (get("txt_encoder_type", "clip_vit_base_16"), get("video_encoder_type", "clip_vit_base_16")):       # modeling.py:298-303
        if t.startswith("clip"):
            clip_type = t
    if clip_type is not None:
        sd.update(clip_to_valor(jit_load(os.path.join(root, PRETRAINED_FILES[clip_type])), int(get("video_resolution", 224))))
    vt = get("video_encoder_type", "clip_vit_base_16")
    if vt.startswith("videoswin"):
        sd.update(swin_to_valor(load(os.path.join(root, PRETRAINED_FILES[vt]))))
    if get("audio_encoder_type", "ast").startswith("ast"):
        sd.update(ast_to_valor(load(os.path.join(root, PRETRAINED_FILES["ast"])), int(get("audio_melbins", 64)),
                               int(get("audio_target_length", 512)), int(get("audio_patch_size", 16))))
    if get("initial_multimodal", True):
        sd.update(bert_to_valor(load(os.path.join(root, PRETRAINED_FILES[get("multimodal_encoder_type", "bert_base_uncased")]))))
    return sd


# ------------------------------------------------------------------------------------------ exact-resume checkpoints of a run
# output_dir/ckpt/model_step_N.pt            model.state_dict(), the reference's keys (utils/save.py:45-49; VALOR.from_pretrained loads it)
#                 optimizer_step_N.pt        the NATIVE optimizer.state_dict(): per-tensor {step, exp_avg, exp_avg_sq} + the fp32 masters
#                 engine_step_N.rank{r}.pt   TrainEngine.state_dict(): step counters and every RNG stream, one file per rank
#                 ema_step_N.pt              WeightEMA.state_dict() of an engine that averages its weights (valor_amd/ema.py), else no
#                                            such file. The name starts with neither `model` nor `optimizer`: the reference's listings
#                                            (train_utils.py:174-187, inference.py:65-66) parse every such name as model_step_N. Its
#                                            "weights" entry is a model checkpoint in the reference's keys, fp32.
# Rank 0 writes the first two and the average. Every file is written under a temporary name (`tmp.<pid>.<name>`: neither latest_step nor the reference's
# `startswith('model')` / `startswith('optimizer')` listings see it) and renamed, so a killed process leaves no half-written step behind.
# Not restored: the position of the data loader (the caller's), and -- for a checkpoint without an engine file, e.g. one the reference
# wrote -- the RNG streams (resume_run(allow_inexact=True)).
_STEP_FILE = {"model": re.compile(r"model_step_(\d+)\.pt"), "optimizer": re.compile(r"optimizer_step_(\d+)\.pt"),
              "engine": re.compile(r"engine_step_(\d+)\.rank(\d+)\.pt"), "ema": re.compile(r"ema_step_(\d+)\.pt")}


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def run_files(output_dir, step, rank=None):
    """the three files of step N for this rank: {'model' | 'optimizer' | 'engine': path}"""
    d = os.path.join(output_dir, "ckpt")
    rank = _rank() if rank is None else rank
    return {"model": os.path.join(d, f"model_step_{step}.pt"), "optimizer": os.path.join(d, f"optimizer_step_{step}.pt"),
            "engine": os.path.join(d, f"engine_step_{step}.rank{rank}.pt")}


def ema_file(output_dir, step):
    """the weight average's file of step N beside the three of run_files: ckpt/ema_step_N.pt"""
    return os.path.join(output_dir, "ckpt", f"ema_step_{step}.pt")


def latest_step(output_dir, rank=None, need_engine=True):
    """load_from_resume's step discovery (train_utils.py:174-187) restated: the largest N for which model_step_N.pt, optimizer_step_N.pt
    and this rank's engine file all exist (need_engine=False: the first two, a checkpoint the reference wrote), or None. Temporary files
    of an interrupted save and steps with a file missing are ignored."""
    d = os.path.join(output_dir, "ckpt")
    if not os.path.isdir(d):
        return None
    rank = _rank() if rank is None else rank
    seen = {k: set() for k in _STEP_FILE}
    for name in os.listdir(d):
        for kind, pat in _STEP_FILE.items():
            m = pat.fullmatch(name)
            if m and (kind != "engine" or int(m.group(2)) == rank):
                seen[kind].add(int(m.group(1)))
    steps = seen["model"] & seen["optimizer"]
    if need_engine:
        steps &= seen["engine"]
    return max(steps) if steps else None


def _write(obj, path):
    tmp = os.path.join(os.path.dirname(path), f"tmp.{os.getpid()}.{os.path.basename(path)}")
    torch.save(obj, tmp)
    os.replace(tmp, path)


def _remove_older(output_dir, step, rank, kinds):
    """opts.remove_before_ckpt (utils/save.py:40-44,60-63) -- but AFTER the new step's files are complete, so there is always one whole
    checkpoint on disk. Rank 0 owns the model / optimizer files, every rank its own engine files."""
    d = os.path.join(output_dir, "ckpt")
    for name in os.listdir(d):
        for kind in kinds:
            m = _STEP_FILE[kind].fullmatch(name)
            if m and int(m.group(1)) != step and (kind != "engine" or int(m.group(2)) == rank):
                os.remove(os.path.join(d, name))


def _host_copy(sd):
    """tensors of a (nested) state dict on the host, compact (a view of the arena becomes a tensor of its own size); keys that alias one
    tensor (the tied decoder weight, txt_encoder.* of the shared BERT) keep sharing one copy"""
    memo = {}

    def go(x):
        if isinstance(x, torch.Tensor):
            key = (x.data_ptr(), tuple(x.shape), tuple(x.stride()), x.dtype, x.device)
            if key not in memo:
                memo[key] = x.detach().cpu().contiguous() if x.device.type != "cpu" else x.detach().clone()
            return memo[key]
        if isinstance(x, dict):
            return {k: go(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return type(x)(go(v) for v in x)
        return x
    return go(sd)


class SaveHandle:
    """what save_run returns: wait() blocks until the files are complete and re-raises what the writer raised"""

    def __init__(self, step, files):
        self.step, self.files, self._thread, self._error = step, files, None, None
        self._t0 = time.perf_counter()
        self.seconds = None               # wall time from the save_run call until the files were complete

    def _finished(self):
        self.seconds = time.perf_counter() - self._t0

    def done(self):
        return self._thread is None or not self._thread.is_alive()

    def wait(self):
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._error is not None:
            err, self._error = self._error, None
            raise err
        return self.step


class _Snapshotter:
    """the non-blocking save of one engine: device-side copies of the flat arenas taken in stream order at the step boundary, moved into
    pinned host memory on a side stream, written by one background thread. Buffers are allocated at the first use and reused; one save
    in flight (the next waits for it)."""

    def __init__(self, engine):
        model, opt = engine.model, engine.optimizer
        self.src = dict(opt.flat_state(), flat=model.arena.flat)       # (fp32 mode: no separate master, the parameters are the masters)
        if getattr(engine, "ema", None) is not None:
            self.src.update(engine.ema.flat_state())                   # the average and its count: the same step boundary
        self.dev = {k: torch.empty_like(t) for k, t in self.src.items()}
        self.host = {k: torch.empty(t.shape, dtype=t.dtype, device="cpu", pin_memory=True) for k, t in self.src.items()}
        self.stream = torch.cuda.Stream(device=model.arena.flat.device)
        self.handle = None

    def wait(self):
        if self.handle is not None:
            h, self.handle = self.handle, None
            h.wait()

    def start(self, engine, handle, engine_sd, after):
        self.wait()
        step, files = handle.step, handle.files
        model, opt = engine.model, engine.optimizer
        cur = torch.cuda.current_stream(model.arena.flat.device)
        for k, t in self.src.items():               # behind step N's optimizer kernels, ahead of step N + 1's: the step's own stream
            self.dev[k].copy_(t)
        taken = torch.cuda.Event()
        taken.record(cur)
        done = torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(taken)
            for k, t in self.dev.items():
                self.host[k].copy_(t, non_blocking=True)
            done.record(self.stream)
        param_groups = [dict(g) for g in opt.param_groups]          # the LR schedule rewrites them at the next step

        def write():
            try:
                done.synchronize()
                if "model" in files:
                    _write(model.state_dict(flat=self.host["flat"]), files["model"])
                    osd = opt.state_dict(flat=self.host)
                    osd["param_groups"] = param_groups
                    _write(osd, files["optimizer"])
                if "ema" in files:
                    _write(engine.ema.state_dict(flat=self.host), files["ema"])
                _write(engine_sd, files["engine"])
                after()
                handle._finished()
            except BaseException as e:          # handed to wait()
                handle._error = e
        handle._thread = threading.Thread(target=write, name=f"valor-ckpt-{step}", daemon=False)
        handle._thread.start()
        self.handle = handle
        return handle


def save_run(engine, output_dir, step=None, blocking=True):
    """Checkpoint a run at a step boundary (layout: the comment above). step: defaults to engine.global_step. Raises RuntimeError inside an
    accumulation window (TrainEngine.state_dict). blocking=False: the call enqueues device-side copies and returns; the returned
    handle's wait() (or the next save_run, or engine.close()) waits for the files. The engine state -- counters, host RNG -- is captured
    at the call in both modes. opts.remove_before_ckpt (default True, utils/save.py:33): older steps' files are removed once the new
    ones are complete."""
    from .ema import refuse_applied
    refuse_applied(engine.model.arena, "checkpoint.save_run")
    step = int(engine.global_step if step is None else step)
    rank = _rank()
    os.makedirs(os.path.join(output_dir, "ckpt"), exist_ok=True)
    saver = getattr(engine, "_saver", None)
    if saver is not None:
        saver.wait()                                  # one save in flight
    engine_sd = engine.state_dict()
    files = run_files(output_dir, step, rank)
    if rank != 0:
        files = {"engine": files["engine"]}
    elif getattr(engine, "ema", None) is not None:
        files["ema"] = ema_file(output_dir, step)
    opts = engine.opts
    remove = bool(opts.get("remove_before_ckpt", True) if isinstance(opts, dict) else getattr(opts, "remove_before_ckpt", True))

    def after():
        if remove:
            _remove_older(output_dir, step, rank, tuple(files))
    handle = SaveHandle(step, files)
    if not blocking and engine.model.arena.flat.is_cuda:
        if saver is None:
            saver = engine._saver = _Snapshotter(engine)
        return saver.start(engine, handle, engine_sd, after)
    if "model" in files:
        _write(_host_copy(engine.model.state_dict()), files["model"])
        _write(_host_copy(engine.optimizer.state_dict()), files["optimizer"])
    if "ema" in files:
        _write(_host_copy(engine.ema.state_dict()), files["ema"])
    _write(engine_sd, files["engine"])
    after()
    handle._finished()
    return handle


def resume_run(engine, output_dir, step=None, allow_inexact=False):
    """Load step N (default: latest_step) into an already constructed model / optimizer / engine and return N: the next train_step
    continues the saved run to the bit (same world size, graphs and token-masker mode; the data loader's position is the caller's).
    A checkpoint without this rank's engine file -- one the reference wrote: its torch-Optimizer file goes through
    FusedAdamW.load_reference_state_dict -- is refused unless allow_inexact=True: then weights, moments and the LR schedule's step
    continue, the RNG streams (dropout masks, token masking, stochastic depth, sampling) start fresh, and the masters are re-derived
    from the parameters. An engine that averages its weights (engine.ema) needs ema_step_N.pt as well: FileNotFoundError without it,
    unless allow_inexact=True -- then the average starts over from the loaded masters with count 0. An engine without an average
    ignores the file."""
    rank = _rank()
    if getattr(engine, "_saver", None) is not None:
        engine._saver.wait()                              # a save of this engine that is still being written
    if step is None:
        step = latest_step(output_dir, rank)
        if step is None and allow_inexact:
            step = latest_step(output_dir, rank, need_engine=False)
        if step is None:
            raise FileNotFoundError(f"resume_run: no complete checkpoint under {os.path.join(output_dir, 'ckpt')}"
                                    + ("" if allow_inexact else " (a step without its engine file needs allow_inexact=True)"))
    files = run_files(output_dir, int(step), rank)
    exact = os.path.exists(files["engine"])
    if not exact and not allow_inexact:
        raise FileNotFoundError(f"resume_run: {files['engine']} is missing -- without it the RNG streams cannot be restored and the run "
                                "does not continue bit-identically; pass allow_inexact=True to continue with fresh RNG state")
    ema = getattr(engine, "ema", None)
    ema_path = ema_file(output_dir, int(step)) if ema is not None else None
    if ema is not None and not os.path.exists(ema_path) and not allow_inexact:
        raise FileNotFoundError(f"resume_run: {ema_path} is missing -- the engine averages its weights and the average cannot be restored; "
                                "pass allow_inexact=True to start it over from the loaded weights")
    engine_sd = torch.load(files["engine"], map_location="cpu", weights_only=True) if exact else None
    if engine_sd is not None:
        engine.load_state_dict(engine_sd)                 # first: it refuses a mismatching run before anything is overwritten
    engine.model.load_state_dict(torch.load(files["model"], map_location="cpu", weights_only=True), strict=True)
    osd = torch.load(files["optimizer"], map_location="cpu", weights_only=True)
    if "names" in osd:
        engine.optimizer.load_state_dict(osd)
    else:                                                 # torch-Optimizer layout: the reference's optimizer_step_N.pt
        engine.optimizer.load_reference_state_dict(osd)
    if ema is not None:
        if os.path.exists(ema_path):
            ema.load_state_dict(torch.load(ema_path, map_location="cpu", weights_only=True))
        else:
            ema.restart()
    if engine_sd is None:
        engine.global_step = int(step)
    return int(step)
