"""CPU: the host side of valor_amd/preprocess.py (slice choice, frame geometry, the numpy filterbank) and the argument validation of
valor_fbank / valor_frames_prepare, which answers before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from valor_amd import preprocess as PP


def _reference_slices(m, T, A):
    """the reference's rule (AudioMapper.__getitem__ + split(), evaluation), written out: pad the m real frames by T - m % T rows, number
    the slices of T rows, repeat the last slice number until there are A, cut the list into A consecutive groups whose sizes differ
    by at most one (the first len % A groups are the larger ones), take the middle element (len + 1) // 2 - 1 of each group"""
    padded = m + (T - m % T)
    numbers = list(range(padded // T))
    while len(numbers) < A:
        numbers.append(numbers[-1])
    base, larger = divmod(len(numbers), A)
    picks = []
    for g in range(A):
        first = g * base + min(g, larger)
        last = (g + 1) * base + min(g + 1, larger)
        group = numbers[first:last]
        picks.append(group[(len(group) + 1) // 2 - 1])
    return picks, len(set(numbers))


@pytest.mark.parametrize("A", [1, 2, 3])
@pytest.mark.parametrize("m", [0, 5, 16, 32, 37])
def test_slice_selection_follows_the_reference_rule(m, A):
    T = 16
    want, nslices = _reference_slices(m, T, A)
    assert PP.audio_slices(m, T, A) == want
    assert nslices == m // T + 1
    if m == 32:
        assert nslices == 3                                   # m % T == 0 appends a whole all-padding slice
        if A == 3:
            assert want == [0, 1, 2]
    if A == 3 and m in (0, 5):
        assert want == [0, 0, 0]                              # one slice, three slots: repeated
    # training: every pick comes from its own group, reproducibly from the generator
    groups = PP.split_groups(m // T + 1, A)
    a = PP.audio_slices(m, T, A, training=True, generator=torch.Generator().manual_seed(5))
    b = PP.audio_slices(m, T, A, training=True, generator=torch.Generator().manual_seed(5))
    assert a == b and all(x in g for x, g in zip(a, groups))


def test_slice_indices_of_a_batch():
    ap = PP.AudioPrep({"audio_melbins": 64, "audio_target_length": 16, "audio_frame_shift": 10}, sample_num=3, device="cpu")
    sl = ap.slice_indices([300, 400 + 31 * 160, None, 400 + 36 * 160 + 7], 16000)
    assert sl.dtype == np.int32 and sl.tolist() == [[0, 0, 0], [0, 1, 2], [-1, -1, -1], [0, 1, 2]]
    assert PP.num_frames(300, 16000) == 0 and PP.num_frames(400 + 31 * 160, 16000) == 32 and PP.num_frames(400 + 36 * 160 + 7, 16000) == 37
    assert PP.fbank_geometry(16000) == (160, 400, 512) and PP.fbank_geometry(44100) == (441, 1102, 2048)


def test_geometry_rows_of_the_three_recipes():
    R = 16
    assert PP.frame_geometry(37, 53, R, "none") == [37, 53, 0, 0, 37, 53, 16, 16, 0, 0, 0]
    assert PP.frame_geometry(53, 37, R, "none") == [53, 37, 0, 0, 53, 37, 16, 16, 0, 0, 0]
    # short side to 16, long side int(16 * 53 / 37) = 22, centre crop offset round((22 - 16) / 2) = 3 on the long axis
    assert PP.frame_geometry(37, 53, R, "crop_flip") == [37, 53, 0, 0, 37, 53, 16, 22, 0, 3, 0]
    assert PP.frame_geometry(53, 37, R, "crop_flip") == [53, 37, 0, 0, 53, 37, 22, 16, 3, 0, 0]
    # training on 37 x 53: a square of area >= 0.8 * 37 * 53 has side >= 39.6 > 37, so all ten attempts fail and the centre fallback
    # (ratio clamped to 1: the full short side) answers
    flips = set()
    for seed in range(16):
        g = torch.Generator().manual_seed(seed)
        row = PP.frame_geometry(37, 53, R, "crop_flip", training=True, generator=g)
        assert row[:10] == [37, 53, 0, 8, 37, 37, 16, 16, 0, 0]
        row2 = PP.frame_geometry(53, 37, R, "crop_flip", training=True, generator=torch.Generator().manual_seed(seed))
        assert row2[:10] == [53, 37, 8, 0, 37, 37, 16, 16, 0, 0]
        flips.add(row[10])
    assert flips == {0, 1}
    # a square source: side = round(sqrt(U(0.8, 1) * 64 * 64)) in [57, 64], anywhere inside
    sides = set()
    for seed in range(32):
        top, left, h, w = PP.random_resized_crop_box(64, 64, generator=torch.Generator().manual_seed(seed))
        assert h == w and 57 <= h <= 64 and 0 <= top <= 64 - h and 0 <= left <= 64 - w
        sides.add(h)
    assert len(sides) > 3
    for row in ([37, 53, 0, 0, 37, 53, 16, 16, 0, 1, 0], [37, 53, 8, 0, 30, 53, 16, 16, 0, 0, 0], [37, 53, 0, 0, 0, 53, 16, 16, 0, 0, 0]):
        with pytest.raises(ValueError):
            PP.check_geometry(row, R)
    vp = PP.VideoPrep({"video_resolution": 16, "video_encoder_type": "clip_vit"}, "crop_flip", device="cpu")
    clips = [[np.zeros((37, 53, 3), np.uint8)] * 2, [np.zeros((53, 37, 3), np.uint8)] * 2]
    assert vp.geometry(clips).tolist() == [[37, 53, 0, 0, 37, 53, 16, 22, 0, 3, 0]] * 2 + [[53, 37, 0, 0, 53, 37, 22, 16, 3, 0, 0]] * 2
    assert vp.mean == PP.CLIP_MEAN and PP.VideoPrep({"video_encoder_type": "videoswin"}, device="cpu").std == PP.IMAGENET_STD


def test_fbank_host_tone_peaks_in_the_nearest_filter():
    sr, melbins = 16000, 64
    t = np.arange(sr // 2, dtype=np.float64) / sr
    fb = PP.fbank_host(0.5 * np.sin(2 * np.pi * 1000.0 * t), sr, 10, melbins, np.float64)
    assert fb.shape == (PP.num_frames(sr // 2, sr), melbins)
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    lo, hi = mel(20.0), mel(sr / 2)
    centres = [lo + (j + 1) * (hi - lo) / (melbins + 1) for j in range(melbins)]
    want = min(range(melbins), key=lambda j: abs(centres[j] - mel(1000.0)))
    assert (fb.argmax(axis=1) == want).all()
    fb32 = PP.fbank_host(0.5 * np.sin(2 * np.pi * 1000.0 * t), sr, 10, melbins, np.float32)
    assert fb32.dtype == np.float32 and (fb32.argmax(axis=1) == want).all()


def test_fbank_host_silence_and_shapes():
    for dt in (np.float32, np.float64):
        fb = PP.fbank_host(np.zeros(400 + 9 * 160), 16000, 10, 32, dt)
        assert fb.shape == (10, 32) and (fb == dt(math.log(float(np.float32(1.1920929e-07))))).all()
    assert PP.fbank_host(np.zeros(300), 16000, 10, 32).shape == (0, 32)
    with pytest.raises(ValueError):
        PP.fbank_host(np.zeros((2, 800)), 16000)
    ap = PP.AudioPrep({}, device="cpu")
    with pytest.raises(ValueError):
        ap.pack([np.zeros((2, 800), np.float32)])
    # int16 PCM stays int16 only if every present clip is
    r, off, lengths = ap.pack([np.ones(5, np.int16), None, np.ones(3, np.int16)])
    assert r.dtype == np.int16 and off.tolist() == [0, 5, 5, 8] and lengths == [5, None, 3]
    r, _, _ = ap.pack([np.ones(5, np.int16), np.ones(3, np.float64)])
    assert r.dtype == np.float32


def test_mel_tables_are_the_dense_weights():
    """each bin feeds at most two filters, the sparse rows reproduce the dense fp64 matrix, the Nyquist bin is not in it"""
    for sr, melbins in ((16000, 64), (44100, 32), (8000, 23)):
        t = PP.fbank_tables(sr, melbins)
        W = PP.mel_weights(sr, melbins, t.P)
        assert W.shape == (melbins, t.P // 2) and ((W > 0).sum(axis=0) <= 2).all()
        dense = np.zeros_like(W)
        st, ptr, w = t.mel_start.numpy(), t.mel_ptr.numpy(), t.mel_w.numpy()
        for j in range(melbins):
            n = ptr[j + 1] - ptr[j]
            assert st[j] + n <= t.P // 2
            dense[j, st[j]:st[j] + n] = w[ptr[j]:ptr[j + 1]]
        assert np.abs(dense - W).max() <= 2.0 ** -24
    with pytest.raises(ValueError):
        PP.fbank_tables(96000, 64)                             # win 2400: P = 4096


def test_no_cpu_fallback():
    from valor_amd import lib
    bp = PP.BatchPrep({"video_resolution": 16, "audio_melbins": 32, "audio_target_length": 16}, device="cpu")
    with pytest.raises(lib.ValorHipError):
        bp.prepare_batch({"frames": [[np.zeros((20, 12, 3), np.uint8)]]})
    with pytest.raises(lib.ValorHipError):
        bp.prepare_batch({"wave": [np.zeros(800, np.float32)]})


def test_argument_validation_without_gpu():
    from valor_amd import lib
    so = lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def fbank(P=512, win=400, melbins=64, T=16, wave=p, out=p, tables=p, std=1.0, A=1, shift=160, offsets=p):
        return so.valor_fbank(None, wave, 0, 16, offsets, p, 1, A, win, shift, P, melbins, T, tables, tables, tables, tables, tables, 8, 0.0, std, out)

    for P, win in ((128, 100), (4096, 2400), (500, 400), (0, 400)):
        assert fbank(P=P, win=win) == -1                      # unsupported FFT size
    assert fbank(P=1024, win=400) == -1 and fbank(P=256, win=400) == -1      # P is not the next power of two of the window
    assert fbank(melbins=0) == -1 and fbank(melbins=-3) == -1 and fbank(melbins=257) == -1
    assert fbank(T=0) == -1 and fbank(A=0) == -1 and fbank(shift=0) == -1 and fbank(std=0.0) == -1
    assert fbank(wave=None) == -1 and fbank(out=None) == -1 and fbank(tables=None) == -1 and fbank(offsets=None) == -1
    assert so.valor_fbank(None, p, 0, 16, p, p, 0, 1, 400, 160, 512, 64, 16, p, p, p, p, p, 8, 0.0, 1.0, p) == 0      # no clips: no-op

    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    std = (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    bad = (ctypes.c_float * 3)(0.25, 0.0, 0.25)

    def frames(R=16, pix=p, off=p, geom=p, out=p, mean=mean, std=std, F=1):
        return so.valor_frames_prepare(None, pix, 64, off, geom, F, R, 0, mean, std, out)

    assert frames(R=0) == -1 and frames(R=-16) == -1 and frames(F=-1) == -1
    assert frames(pix=None) == -1 and frames(off=None) == -1 and frames(geom=None) == -1 and frames(out=None) == -1
    assert frames(mean=None) == -1 and frames(std=None) == -1 and frames(std=bad) == -1
    assert frames(F=0) == 0
