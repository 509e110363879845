"""Time the device-side input preparation against the reference's host recipe on one batch:
64 clips of 8 frames at 360 x 640 and 10 s of 16 kHz audio -> video_pixels [64, 8, 3, 224, 224], audio_spectrograms [64, 1, 64, 512].

device: the two launches alone (valor_frames_prepare, valor_fbank; device events over --iters launches on staged inputs) and the whole
        prepare_batch call (packing into pinned memory + one H2D copy and one launch per modality; host clock around a synchronise).
host:   the same work as the reference does it, on --threads CPU threads: per clip F.interpolate(bilinear) + normalise of the frames and
        fbank_host in fp32 (+ pad / slice / normalise) of the waveform.

Writes one JSON line to --out (default profiles/preproc_bench.json) and prints it. No pass / fail bar: a measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from valor_amd import kernels as K                # noqa: E402
from valor_amd import preprocess as PP            # noqa: E402


def host_batch(frames, waves, prep, sr):
    mean = torch.tensor(prep.video.mean)[None, :, None, None]
    std = torch.tensor(prep.video.std)[None, :, None, None]
    R, T, ap = prep.video.resolution, prep.audio.target_length, prep.audio
    vids, auds = [], []
    for clip, wave in zip(frames, waves):
        x = torch.from_numpy(np.stack(clip)).permute(0, 3, 1, 2).float() / 255
        vids.append((F.interpolate(x, size=(R, R), mode="bilinear", align_corners=False) - mean) / std)
        fb = PP.fbank_host(wave, sr, ap.frame_shift, ap.melbins, np.float32)
        m = fb.shape[0]
        fb = np.concatenate([fb, np.zeros((T - m % T, ap.melbins), np.float32)])
        sl = PP.audio_slices(m, T, ap.sample_num)
        out = np.stack([fb[s * T:(s + 1) * T] for s in sl]).transpose(0, 2, 1)
        auds.append((out - np.float32(ap.mean)) / np.float32(2 * ap.std))
    return torch.stack(vids), torch.from_numpy(np.stack(auds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preproc_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_preproc.py measures on the GPU"
    torch.set_num_threads(a.threads)
    dev, sr = torch.device("cuda:0"), 16000
    rng = np.random.default_rng(0)
    frames = [[rng.integers(0, 256, size=(a.height, a.width, 3), dtype=np.uint8) for _ in range(a.frames)] for _ in range(a.clips)]
    waves = [(0.1 * rng.standard_normal(int(a.seconds * sr)) + 0.05).astype(np.float32) for _ in range(a.clips)]
    opts = {"video_resolution": 224, "video_encoder_type": "clip", "audio_melbins": 64, "audio_target_length": 512,
            "audio_mean": -4.2677393, "audio_std": 4.5689974, "audio_frame_shift": 10}
    prep = PP.BatchPrep(opts, "none", training=False, device=dev, audio_sample_num=1)
    raw = {"frames": frames, "wave": waves, "sample_rate": sr}

    # whole call (pack + copy + launch), warmed
    for _ in range(2):
        out = prep.prepare_batch(raw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        out = prep.prepare_batch(raw)
    torch.cuda.synchronize()
    call_ms = (time.perf_counter() - t0) / reps * 1e3

    # the launches alone, on staged inputs
    flat = [f for c in frames for f in c]
    geom = torch.from_numpy(prep.video.geometry(frames)).to(dev)
    offs = np.zeros(len(flat), np.int64)
    np.cumsum([f.size for f in flat[:-1]], out=offs[1:])
    pix = torch.from_numpy(np.concatenate([f.reshape(-1) for f in flat])).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    _, woffs, lengths = prep.audio.pack(waves)
    d_wave, d_woffs = torch.from_numpy(np.concatenate(waves)).to(dev), torch.from_numpy(woffs).to(dev)
    d_sl = torch.from_numpy(prep.audio.slice_indices(lengths, sr)).to(dev)
    tables = prep.audio.tables(sr)
    vout = torch.empty((len(flat), 3, 224, 224), device=dev)
    aout = torch.empty((a.clips, 1, 64, 512), device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    frames_ms = timed(lambda: K.frames_prepare(pix, d_offs, geom, 224, prep.video.mean, prep.video.std, out=vout))
    fbank_ms = timed(lambda: K.fbank(d_wave, d_woffs, d_sl, tables, 64, 512, prep.audio.mean, prep.audio.std, out=aout))
    frames_aa_ms = timed(lambda: K.frames_prepare(pix, d_offs, geom, 224, prep.video.mean, prep.video.std, antialias=True, out=vout))

    host_batch(frames[:2], waves[:2], prep, sr)
    t0 = time.perf_counter()
    hv, ha = host_batch(frames, waves, prep, sr)
    host_ms = (time.perf_counter() - t0) * 1e3
    dv = float((out["video_pixels"].cpu() - hv.view_as(out["video_pixels"])).abs().max())
    da = float((out["audio_spectrograms"].cpu() - ha).abs().max())

    in_bytes, out_bytes = pix.numel() + d_wave.numel() * 4, (vout.numel() + aout.numel()) * 4
    res = {"bench": "preproc", "clips": a.clips, "frames": a.frames, "source": [a.height, a.width], "seconds": a.seconds, "sample_rate": sr,
           "frames_prepare_ms": round(frames_ms, 4), "frames_prepare_antialias_ms": round(frames_aa_ms, 4), "fbank_ms": round(fbank_ms, 4),
           "prepare_batch_call_ms": round(call_ms, 2), "host_ms": round(host_ms, 1), "host_threads": a.threads,
           "device_samples_per_s": round(a.clips / ((frames_ms + fbank_ms) * 1e-3), 1), "host_samples_per_s": round(a.clips / (host_ms * 1e-3), 1),
           "input_MB": round(in_bytes / 1e6, 1), "output_MB": round(out_bytes / 1e6, 1),
           "frames_prepare_GBps": round((pix.numel() + vout.numel() * 4) / frames_ms / 1e6, 1),
           "max_abs_diff_vs_host": {"video_pixels": dv, "audio_spectrograms": da}, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
