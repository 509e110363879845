"""GPU: valor_fbank and valor_frames_prepare (valor_amd/csrc/preproc.hip) against fp64 host references, at the smallest shapes where
each rule can break, and prepare_batch end to end into the encoders.

Tolerances come from the references, not from the kernels: four times the largest deviation of the SAME host computation in fp32
from its fp64 run on the test's inputs (the factor covers the different summation order of an FFT / of the mel sums, and of the
separable resampling). Each test prints the figure it saw before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from valor_amd import preprocess as PP

pytestmark = pytest.mark.gpu

MEAN, STD = -4.2677393, 4.5689974
LOG_EPS = np.float32(math.log(float(np.float32(1.1920929e-07))))


def _noise(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n) + 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _clips(sr):
    """the clips of one launch (None = absent) and, per melbins, their fp64 / fp32 host filterbanks (computed once, shared)"""
    if sr == 16000:
        return (_noise(300, 1), _noise(400 + 31 * 160, 2), _noise(400 + 36 * 160 + 7, 3), None, np.zeros(400 + 20 * 160, np.float32))
    return (_noise(1102 + 17 * 441 + 5, 4), _noise(1000, 5), None)


@functools.lru_cache(maxsize=None)
def _host(sr, melbins):
    fb64 = [None if c is None else PP.fbank_host(c, sr, 10, melbins, np.float64) for c in _clips(sr)]
    fb32 = [None if c is None else PP.fbank_host(c, sr, 10, melbins, np.float32) for c in _clips(sr)]
    dev = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(fb32, fb64) if a is not None and a.size)
    return fb64, dev


def _reference_audio(fb, slices, T, melbins):
    """AudioMapper.__getitem__ from the fbank on, in fp64: zero rows up to m + (T - m % T), the chosen slices, [A, melbins, T], normalise"""
    if fb is None:
        return np.zeros((len(slices), melbins, T))
    m = fb.shape[0]
    padded = np.concatenate([fb, np.zeros((T - m % T, melbins))], axis=0)
    out = np.stack([padded[s * T:(s + 1) * T] for s in slices], axis=0).transpose(0, 2, 1)
    return (out - MEAN) / (STD * 2)


def _f32_norm(v):
    return (np.float32(v) - np.float32(MEAN)) / (np.float32(2) * np.float32(STD))


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("melbins", [64, 32])
def test_fbank_16k(dev, melbins, A):
    T, sr = 16, 16000
    clips = _clips(sr)
    ap = PP.AudioPrep({"audio_melbins": melbins, "audio_target_length": T, "audio_mean": MEAN, "audio_std": STD, "audio_frame_shift": 10},
                      sample_num=A, device=dev)
    out = ap(list(clips), sr=sr)
    torch.cuda.synchronize()
    assert out.shape == (len(clips), A, melbins, T) and out.dtype == torch.float32 and out.is_cuda
    got = out.cpu().numpy()
    fb64, host_dev = _host(sr, melbins)
    sl = ap.slice_indices([None if c is None else c.size for c in clips], sr)
    ref = np.stack([_reference_audio(fb, s, T, melbins) for fb, s in zip(fb64, sl.tolist())])
    tol = 4 * host_dev / (2 * STD)
    # the all-zero clip and padding are exact (below); the bound is about the noise clips
    err = float(np.abs(got.astype(np.float64) - ref)[[0, 1, 2]].max())
    print(f"fbank 16 kHz melbins={melbins} A={A}: device vs fp64 {err * 2 * STD:.3e} log units, fp32 host vs fp64 {host_dev:.3e}, bound {4 * host_dev:.3e}")
    assert np.isfinite(got).all()
    assert err <= tol
    pad = _f32_norm(0.0)
    assert (got[0] == pad).all()                              # N = 300 < a window: one slice of padding rows
    assert (got[3] == 0.0).all()                              # absent: the reference's torch.zeros
    assert sl[1].tolist() == ([1] if A == 1 else [0, 1, 2])   # m = 32: three slices, the last all padding
    if A == 3:
        assert (got[1, 2] == pad).all() and (got[2, 2, :, 5:] == pad).all() and (got[2, 2, :, :5] != pad).all()   # m = 37: 5 real rows in slice 2
    # all-zero audio: every real frame sits on the floor; 21 frames = slice 0 full, slice 1 five rows
    z = got[4]
    zs = sl[4].tolist()
    for a, s in enumerate(zs):
        real = max(0, min(T, 21 - s * T))
        assert (z[a, :, :real] == _f32_norm(LOG_EPS)).all() and (z[a, :, real:] == pad).all()


def test_fbank_44k(dev):
    T, sr, melbins, A = 8, 44100, 64, 2
    clips = _clips(sr)
    ap = PP.AudioPrep({"audio_melbins": melbins, "audio_target_length": T, "audio_mean": MEAN, "audio_std": STD}, sample_num=A, device=dev)
    assert ap.tables(sr).P == 2048 and ap.tables(sr).win == 1102
    got = ap(list(clips), sr=sr).cpu().numpy()
    fb64, host_dev = _host(sr, melbins)
    sl = ap.slice_indices([None if c is None else c.size for c in clips], sr)
    assert sl.tolist() == [[0, 2], [0, 0], [-1, -1]]          # 18 frames: slices 0, 1, 2 in the groups [0, 1] and [2]; 1000 samples: no frame
    ref = np.stack([_reference_audio(fb, s, T, melbins) for fb, s in zip(fb64, sl.tolist())])
    err = float(np.abs(got.astype(np.float64) - ref)[[0]].max())
    print(f"fbank 44.1 kHz: device vs fp64 {err * 2 * STD:.3e} log units, fp32 host vs fp64 {host_dev:.3e}, bound {4 * host_dev:.3e}")
    assert err <= 4 * host_dev / (2 * STD)
    assert (got[1] == _f32_norm(0.0)).all() and (got[2] == 0.0).all()


def test_fbank_pcm16_equals_fp32(dev):
    """int16 PCM and the same samples as fp32 (q / 32768, exact) give bit-identical output"""
    T, sr = 16, 16000
    q = np.clip(np.round(_noise(400 + 36 * 160 + 7, 6) * 32768.0), -32768, 32767).astype(np.int16)
    ap = PP.AudioPrep({"audio_melbins": 64, "audio_target_length": T, "audio_mean": MEAN, "audio_std": STD}, sample_num=3, device=dev)
    a = ap([q, None, q[:3000]], sr=sr)
    b = ap([q.astype(np.float32) / np.float32(32768.0), None, q[:3000].astype(np.float32) / np.float32(32768.0)], sr=sr)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    fb = PP.fbank_host(q, sr, 10, 64, np.float64)
    host_dev = float(np.abs(PP.fbank_host(q, sr, 10, 64, np.float32) - fb).max())
    assert np.abs(a[0].cpu().numpy() - _reference_audio(fb, [0, 1, 2], T, 64)).max() <= 4 * host_dev / (2 * STD)


# ---------------------------------------------------------------- frames
def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _reference_frame(img, row, R, antialias, mean, std, dtype):
    """the recipe on the host: crop, F.interpolate to the virtual size, the R x R window, normalise, flip"""
    H, W, top, left, h, w, Hv, Wv, oy, ox, flip = row
    x = torch.from_numpy(img).permute(2, 0, 1).to(dtype) / 255
    x = x[:, top:top + h, left:left + w]
    y = F.interpolate(x[None], size=(Hv, Wv), mode="bilinear", align_corners=False, antialias=antialias)[0][:, oy:oy + R, ox:ox + R]
    return y, flip


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("R", [16, 32, 33])
def test_frames_prepare(dev, R, antialias):
    from valor_amd import kernels as K
    big, small, sq = _frame(37, 53, 1), _frame(20, 12, 2), _frame(33, 33, 3)
    frames, rows = [], []
    for img in (big, small, sq):
        H, W = img.shape[:2]
        frames += [img, img]
        rows += [PP.frame_geometry(H, W, R, "none"), PP.frame_geometry(H, W, R, "crop_flip")]      # full box; short side + centre crop
    frames += [big, small]
    rows += [[37, 53, 3, 11, 30, 30, R, R, 0, 0, 1], [20, 12, 0, 0, 20, 12, R, R, 0, 0, 1]]          # a crop box with flip; a flipped upscale
    for row in rows:
        PP.check_geometry(row, R)
    offsets = np.zeros(len(frames), np.int64)
    np.cumsum([f.size for f in frames[:-1]], out=offsets[1:])
    pix = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(dev)
    out = K.frames_prepare(pix, torch.from_numpy(offsets).to(dev), torch.tensor(rows, dtype=torch.int32, device=dev), R, PP.CLIP_MEAN, PP.CLIP_STD,
                           antialias=antialias)
    torch.cuda.synchronize()
    assert out.shape == (len(frames), 3, R, R) and out.dtype == torch.float32
    got = out.cpu().double()
    mean, std = torch.tensor(PP.CLIP_MEAN, dtype=torch.float64)[:, None, None], torch.tensor(PP.CLIP_STD, dtype=torch.float64)[:, None, None]
    host_dev, err = 0.0, torch.zeros(3, dtype=torch.float64)
    for i, (img, row) in enumerate(zip(frames, rows)):
        y64, flip = _reference_frame(img, row, R, antialias, mean, std, torch.float64)
        y32, _ = _reference_frame(img, row, R, antialias, mean, std, torch.float32)
        host_dev = max(host_dev, float((y32.double() - y64).abs().max()))
        ref = (y64 - mean) / std
        if flip:
            ref = ref.flip(-1)
        err = torch.maximum(err, (got[i] - ref).abs().amax(dim=(1, 2)))
    print(f"frames R={R} antialias={antialias}: device vs fp64 per channel {[f'{float(e):.3e}' for e in err]} (after / std), "
          f"fp32 host vs fp64 {host_dev:.3e} (before / std)")
    assert torch.isfinite(got).all()
    for c in range(3):
        assert float(err[c]) <= 4 * host_dev / PP.CLIP_STD[c]
    if R == 33:                                  # 33 x 33 -> 33: the identity, exact to the one rounding of the result
        want = ((torch.from_numpy(sq).permute(2, 0, 1).double() / 255 - mean) / std).float()
        assert (got[4].float() - want).abs().max() <= float(torch.finfo(torch.float32).eps) * float(want.abs().max())


def test_frames_bad_geometry_is_nan_not_a_fault(dev):
    """a row that points outside its frame reads nothing (the Python layer refuses it earlier; this is the kernel's own guard)"""
    from valor_amd import kernels as K
    img = _frame(20, 12, 4)
    rows = torch.tensor([[20, 12, 0, 0, 20, 12, 16, 16, 0, 0, 0], [20, 12, 5, 0, 20, 12, 16, 16, 0, 0, 0], [20, 12, 0, 0, 20, 12, 16, 16, 0, 1, 0]],
                        dtype=torch.int32, device=dev)
    out = K.frames_prepare(torch.from_numpy(img.reshape(-1)).to(dev), torch.zeros(3, dtype=torch.int64, device=dev), rows, 16, PP.CLIP_MEAN, PP.CLIP_STD)
    assert torch.isfinite(out[0]).all() and torch.isnan(out[1]).all() and torch.isnan(out[2]).all()


# ---------------------------------------------------------------- end to end
def test_prepare_batch_feeds_the_encoders(dev):
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    spec = synth.tiny_spec()
    opts = {"video_resolution": spec.resolution, "video_encoder_type": "clip", "audio_melbins": spec.melbins,
            "audio_target_length": spec.target_len, "audio_mean": MEAN, "audio_std": STD, "audio_frame_shift": 10}
    bp = PP.BatchPrep(opts, "crop_flip", training=False, device=dev, audio_sample_num=2)
    raw = {"frames": [[_frame(48, 80, 10 + i) for i in range(2)], [_frame(70, 66, 20 + i) for i in range(2)]],
           "wave": [_noise(400 + 100 * 160, 7), None], "sample_rate": 16000, "ids": ["a", "b"]}
    batch = bp.prepare_batch(raw)
    v, a = batch["video_pixels"], batch["audio_spectrograms"]
    assert batch["ids"] == ["a", "b"] and "frames" not in batch and "wave" not in batch
    assert v.shape == (2, 2, 3, spec.resolution, spec.resolution) and v.dtype == torch.float32 and v.is_cuda
    assert a.shape == (2, 2, spec.melbins, spec.target_len) and a.dtype == torch.float32 and a.is_cuda
    assert torch.isfinite(v).all() and torch.isfinite(a).all() and (a[1] == 0).all()
    model = VALOR({"dropout": 0.0, "drop_path_rate": 0.0}, spec=spec, dtype=torch.float32, device=dev)
    model.load_state_dict(synth.make_state_dict(spec, seed=3, w_std=0.05), strict=True)
    model.eval()
    with torch.no_grad():
        vo, ao = model.forward_video_encoder(v), model.forward_audio_encoder(a)
    assert vo.shape[:2] == (2, 2) and ao.shape[:2] == (2, 2)
    assert torch.isfinite(vo.float()).all() and torch.isfinite(ao.float()).all()
    side = torch.cuda.Stream(device=dev)
    again = bp.prepare_batch(raw, stream=side)
    torch.cuda.synchronize()
    assert torch.equal(again["video_pixels"], v) and torch.equal(again["audio_spectrograms"], a)
