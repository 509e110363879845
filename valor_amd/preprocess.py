"""Input preparation: decoded RGB frames and PCM waveforms -> the model's `video_pixels` [B, n, 3, R, R] and `audio_spectrograms`
[B, A, melbins, T], on the device (valor_amd/csrc/preproc.hip). This is the tensor work of the reference's VideoMapper / AudioMapper
(data/data.py:135-323); reading files and tokenisation stay with the dataset.

The host does the small integer work only: which T-frame slice of a clip's padded fbank goes to which output slot (the reference's
split() rule), the crop box / flip of a clip (torchvision's RandomResizedCrop.get_params law) and the fp64 tables of the filterbank.
Random choices come from a passed torch.Generator: the reference's LAW, not the draw order of its `random` module.

fbank_host() restates the filterbank law in numpy for tests and for checking a dataset. Nothing calls it implicitly: there is no
fallback (valor_amd/lib.py); without the library or a GPU, prepare_batch raises.
"""
import math

import numpy as np
import torch

FBANK_EPS = float(np.finfo(np.float32).eps)        # 1.1920929e-07, the floor torchaudio puts under the mel energies
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GEOM_FIELDS = ("H", "W", "top", "left", "h", "w", "Hv", "Wv", "oy", "ox", "flip")


def _opt(opts, name, default=None):
    if isinstance(opts, dict):
        return opts.get(name, default)
    return getattr(opts, name, default)


# ---------------------------------------------------------------- filterbank law
def fbank_geometry(sr, frame_shift_ms=10):
    """(shift, win, P): samples per hop, samples per 25 ms window, the FFT size (next power of two >= win)"""
    shift, win = int(sr * 0.001 * frame_shift_ms), int(sr * 0.001 * 25)
    if shift <= 0 or win < 2:
        raise ValueError(f"sample rate {sr} / frame shift {frame_shift_ms} ms leave no frame")
    P = 1 << (win - 1).bit_length()
    return shift, win, P


def num_frames(n_samples, sr, frame_shift_ms=10):
    """snip_edges framing: 1 + (N - win) // shift, 0 for a clip shorter than a window"""
    shift, win, _ = fbank_geometry(sr, frame_shift_ms)
    return 1 + (n_samples - win) // shift if n_samples >= win else 0


def _mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_weights(sr, melbins, P):
    """fp64 [melbins, P/2]: triangular filters on the mel scale from 20 Hz to Nyquist, melbins + 2 equally spaced edges, evaluated at the
    FFT bin frequencies i * sr / P, i < P/2 (the Nyquist bin has weight 0 and is left out)"""
    lo, hi = _mel(20.0), _mel(0.5 * sr)
    delta = (hi - lo) / (melbins + 1)
    j = np.arange(melbins, dtype=np.float64)[:, None]
    left, center, right = lo + j * delta, lo + (j + 1.0) * delta, lo + (j + 2.0) * delta
    mel = _mel(np.arange(P // 2, dtype=np.float64) * (sr / P))[None, :]
    return np.maximum(0.0, np.minimum((mel - left) / (center - left), (right - mel) / (right - center)))


def hann_window(win):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / (win - 1))


class FbankTables:
    """the host-built fp64 tables of valor_fbank (the mel weights rounded once to fp32) for one (sample rate, melbins, frame shift)"""

    def __init__(self, sr, melbins, frame_shift_ms=10):
        self.sr, self.melbins, self.frame_shift_ms = int(sr), int(melbins), frame_shift_ms
        self.shift, self.win, self.P = fbank_geometry(sr, frame_shift_ms)
        if self.P not in (256, 512, 1024, 2048):
            raise ValueError(f"sample rate {sr}: FFT size {self.P} is outside 256 .. 2048 (8 kHz .. 48 kHz)")
        if not 0 < self.melbins <= 256:
            raise ValueError(f"audio_melbins {melbins} outside 1 .. 256")
        W = mel_weights(sr, melbins, self.P)
        start, ptr, vals = [], [0], []
        for row in W:
            nz = np.nonzero(row)[0]
            a, b = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)        # a triangle's support is one run of bins
            start.append(a)
            vals.append(row[a:b])
            ptr.append(ptr[-1] + b - a)
        k = np.arange(self.P // 2, dtype=np.float64)
        ang = 2.0 * np.pi * k / self.P
        self.window = torch.from_numpy(hann_window(self.win))
        self.twiddle = torch.from_numpy(np.stack([np.cos(ang), -np.sin(ang)], axis=1))
        self.mel_start = torch.tensor(start, dtype=torch.int32)
        self.mel_ptr = torch.tensor(ptr, dtype=torch.int32)
        self.mel_w = torch.from_numpy(np.concatenate(vals + [np.zeros(1)]).astype(np.float32))   # (one spare entry: never empty)

    def to_device(self, device):
        for k in ("window", "twiddle", "mel_start", "mel_ptr", "mel_w"):
            setattr(self, k, getattr(self, k).to(device))
        return self


def fbank_tables(sr, melbins, frame_shift_ms=10):
    return FbankTables(sr, melbins, frame_shift_ms)


def fbank_host(wave, sr, frame_shift_ms=10, melbins=64, dtype=np.float32):
    """kaldi.fbank(htk_compat=True, use_energy=False, window_type='hanning', dither=0) of `wave - wave.mean()` in numpy, every step in
    `dtype` (fp32 or fp64; the tables are built in fp64 and rounded to it): [m, melbins] log mel energies, before the reference's padding
    and normalisation. The DFT is written as two matrix products, so the fp32 result carries the rounding of plain fp32 sums."""
    wave = np.asarray(wave)
    if wave.ndim != 1:
        raise ValueError("mono audio only: the waveform must be 1-D")
    if wave.dtype == np.int16:
        wave = wave.astype(np.float64) / 32768.0
    dt = np.dtype(dtype)
    shift, win, P = fbank_geometry(sr, frame_shift_ms)
    x = wave.astype(dt)
    m = 1 + (x.size - win) // shift if x.size >= win else 0
    if m == 0:
        return np.zeros((0, melbins), dtype=dt)
    x = x - x.mean(dtype=dt)
    fr = np.lib.stride_tricks.as_strided(x, shape=(m, win), strides=(x.strides[0] * shift, x.strides[0])).astype(dt)
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=dt)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = (fr - dt.type(0.97) * prev) * hann_window(win).astype(dt)[None, :]
    ang = 2.0 * np.pi * np.outer(np.arange(win, dtype=np.float64), np.arange(P // 2, dtype=np.float64)) / P   # zero padding: rows >= win drop out
    re, im = fr @ np.cos(ang).astype(dt), fr @ np.sin(ang).astype(dt)
    power = re * re + im * im
    e = power @ mel_weights(sr, melbins, P).T.astype(dt)
    return np.log(np.maximum(e, dt.type(FBANK_EPS))).astype(dt)


# ---------------------------------------------------------------- the reference's choice rules
def split_groups(count, sample_num):
    """the reference's split(): `count` items (0 .. count - 1) in `sample_num` consecutive groups whose sizes differ by at most one, the
    larger groups first; fewer items than groups: the last item is repeated until there is one per group"""
    if count <= 0 or sample_num <= 0:
        raise ValueError("split_groups needs at least one item and one group")
    items = list(range(count)) + [count - 1] * max(0, sample_num - count)
    size, extra = divmod(len(items), sample_num)
    groups, at = [], 0
    for g in range(sample_num):
        n = size + (1 if g < extra else 0)
        groups.append(items[at:at + n])
        at += n
    return groups


def choose(groups, training, generator=None):
    """one element per group: the middle one (evaluation) or a uniform draw from `generator` (training)"""
    if not training:
        return [g[(len(g) + 1) // 2 - 1] for g in groups]
    return [g[int(torch.randint(len(g), (1,), generator=generator))] for g in groups]


def audio_slices(m, T, sample_num, training=False, generator=None):
    """which T-frame slices of a clip of m real frames go to the sample_num output slots. The reference pads to m + (T - m % T) rows,
    i.e. m // T + 1 slices (a whole all-padding slice when m % T == 0)."""
    return choose(split_groups(m // T + 1, sample_num), training, generator)


def _uniform(lo, hi, generator):
    return lo + (hi - lo) * float(torch.rand((), generator=generator, dtype=torch.float64))


def random_resized_crop_box(H, W, scale=(0.8, 1.0), ratio=(1.0, 1.0), generator=None):
    """torchvision's RandomResizedCrop.get_params law: (top, left, h, w). Ten attempts at area ~ U(scale) * H * W and log-uniform
    aspect ratio; then the centre fallback at the nearest admissible ratio."""
    area = H * W
    for _ in range(10):
        target = area * _uniform(scale[0], scale[1], generator)
        aspect = math.exp(_uniform(math.log(ratio[0]), math.log(ratio[1]), generator))
        w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            top = int(torch.randint(0, H - h + 1, (1,), generator=generator))
            left = int(torch.randint(0, W - w + 1, (1,), generator=generator))
            return top, left, h, w
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def frame_geometry(H, W, R, video_transforms="none", training=False, generator=None):
    """the geometry row of valor_frames_prepare (GEOM_FIELDS) of one clip's frames under the three recipes of VideoMapper:
    'none': Resize((R, R)); 'crop_flip' evaluation: Resize(R) (short side to R, long side to int(R * long / short)) + CenterCrop(R);
    'crop_flip' training: RandomResizedCrop(R, [0.8, 1], [1, 1]) + RandomHorizontalFlip."""
    if video_transforms == "none":
        return [H, W, 0, 0, H, W, R, R, 0, 0, 0]
    if video_transforms != "crop_flip":
        raise NotImplementedError(video_transforms)
    if training:
        top, left, h, w = random_resized_crop_box(H, W, generator=generator)
        flip = int(float(torch.rand((), generator=generator)) < 0.5)
        return [H, W, top, left, h, w, R, R, 0, 0, flip]
    if W <= H:
        Wv, Hv = R, int(R * H / W)
    else:
        Hv, Wv = R, int(R * W / H)
    return [H, W, 0, 0, H, W, Hv, Wv, int(round((Hv - R) / 2.0)), int(round((Wv - R) / 2.0)), 0]


def check_geometry(row, R):
    H, W, top, left, h, w, Hv, Wv, oy, ox, _ = row
    if not (H > 0 and W > 0 and h > 0 and w > 0 and 0 <= top and top + h <= H and 0 <= left and left + w <= W and
            0 <= oy and oy + R <= Hv and 0 <= ox and ox + R <= Wv):
        raise ValueError(f"frame geometry {dict(zip(GEOM_FIELDS, row))} does not fit resolution {R}")


# ---------------------------------------------------------------- packed pinned staging
class _PinnedRing:
    """two pinned byte buffers used in turn; a buffer is rewritten only after the copy that last read it has executed"""

    def __init__(self):
        self.bufs, self.events, self.flip = [None, None], [None, None], 0

    def take(self, nbytes):
        i = self.flip
        self.flip ^= 1
        if self.events[i] is not None:
            self.events[i].synchronize()
            self.events[i] = None
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        return i, self.bufs[i]

    def sent(self, i, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        self.events[i] = ev


def _align(n, a=16):
    return (n + a - 1) // a * a


class _Region:
    """arrays of one dtype written back to back into the staging buffer (no intermediate concatenation)"""

    def __init__(self, dtype, arrays):
        self.dtype, self.arrays = np.dtype(dtype), arrays
        self.nbytes = sum(a.size for a in arrays) * self.dtype.itemsize

    def write(self, dst):
        at = 0
        for a in self.arrays:
            n = a.size * self.dtype.itemsize
            dst[at:at + n] = np.ascontiguousarray(a, dtype=self.dtype).reshape(-1).view(np.uint8)
            at += n


def _pack(ring, parts, device, stream):
    """parts: numpy arrays / _Region -> device views of ONE pinned buffer sent with ONE asynchronous copy on `stream`"""
    offs, at = [], 0
    for p in parts:
        offs.append(at)
        at = _align(at + p.nbytes)
    slot, buf = ring.take(at)
    host = buf.numpy()
    for p, o in zip(parts, offs):
        if isinstance(p, _Region):
            p.write(host[o:o + p.nbytes])
        else:
            host[o:o + p.nbytes] = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
    dev = buf[:at].to(device, non_blocking=True)
    ring.sent(slot, stream)
    views = []
    for p, o in zip(parts, offs):
        v = dev[o:o + p.nbytes]
        views.append(v if p.dtype == np.uint8 else v.view(getattr(torch, np.dtype(p.dtype).name)))
    return views


class _Prep:
    def __init__(self, device, training, generator):
        self.device = torch.device(device)
        self.training, self.generator = bool(training), generator
        self._ring = _PinnedRing()

    def _need_gpu(self):
        from . import lib
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise lib.ValorHipError("valor_amd.preprocess runs on the GPU (no CPU fallback); fbank_host is the explicit host restatement")


class AudioPrep(_Prep):
    """AudioMapper's tensor work on the device. opts: audio_melbins, audio_target_length, audio_mean, audio_std, audio_frame_shift (the
    reference's names; audio_sample_num = the slices per clip, A). The reference's 'ast' mapper overrides the target length with 512;
    here the option is taken as given."""

    def __init__(self, opts, sample_num=None, training=False, device="cuda", generator=None):
        super().__init__(device, training, generator)
        self.melbins = int(_opt(opts, "audio_melbins", 64))
        self.target_length = int(_opt(opts, "audio_target_length", 512))
        self.mean, self.std = float(_opt(opts, "audio_mean", -4.2677393)), float(_opt(opts, "audio_std", 4.5689974))
        self.frame_shift = _opt(opts, "audio_frame_shift", 10)
        self.sample_num = int(sample_num if sample_num is not None else _opt(opts, "audio_sample_num", 1))
        if self.melbins <= 0 or self.target_length <= 0 or self.sample_num <= 0 or self.std == 0:
            raise ValueError("audio_melbins, audio_target_length, the slice count must be positive and audio_std non-zero")
        self._tables = {}

    def tables(self, sr):
        key = (int(sr), self.melbins, self.frame_shift)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = FbankTables(sr, self.melbins, self.frame_shift).to_device(self.device)
        return t

    def slice_indices(self, lengths, sr):
        """int32 [B, A]: the slice per output slot of clips of `lengths` samples (None: no audio, -1)"""
        rows = []
        for n in lengths:
            if n is None:
                rows.append([-1] * self.sample_num)
            else:
                rows.append(audio_slices(num_frames(n, sr, self.frame_shift), self.target_length, self.sample_num, self.training, self.generator))
        return np.asarray(rows, dtype=np.int32).reshape(len(rows), self.sample_num)

    def pack(self, waves):
        """(the samples as a staging region, int64 offsets [B + 1], lengths with None for absent clips): int16 if every clip is int16 PCM,
        else fp32"""
        arrs = []
        for w in waves:
            if w is None:
                arrs.append(None)
                continue
            w = w.numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
            if w.ndim != 1:
                raise ValueError("mono audio only: a waveform must be 1-D")
            if w.dtype != np.int16 and w.dtype != np.float32:
                if not np.issubdtype(w.dtype, np.floating):
                    raise ValueError(f"waveform dtype {w.dtype}: int16 PCM or floating point in [-1, 1]")
                w = w.astype(np.float32)
            arrs.append(w)
        present = [w for w in arrs if w is not None]
        pcm = bool(present) and all(w.dtype == np.int16 for w in present)
        if not pcm:
            present = [w.astype(np.float32) / np.float32(32768.0) if w.dtype == np.int16 else w for w in present]
        it = iter(present)
        arrs = [None if w is None else next(it) for w in arrs]
        lengths = [None if w is None else int(w.size) for w in arrs]
        offsets = np.zeros(len(arrs) + 1, dtype=np.int64)
        np.cumsum([0 if n is None else n for n in lengths], out=offsets[1:])
        return _Region(np.int16 if pcm else np.float32, present), offsets, lengths

    def __call__(self, waves, sr=16000, stream=None):
        """waves: per clip a 1-D int16 / float array or None -> audio_spectrograms fp32 [B, A, melbins, T] on the device"""
        from . import kernels as K
        self._need_gpu()
        data, offsets, lengths = self.pack(waves)
        sl = self.slice_indices(lengths, sr)
        tables = self.tables(sr)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            d_off, d_sl, d_wave = _pack(self._ring, [offsets, sl, data], self.device, s)
            return K.fbank(d_wave, d_off, d_sl.view(sl.shape), tables, self.melbins, self.target_length, self.mean, self.std)


class VideoPrep(_Prep):
    """VideoMapper's tensor work on the device. opts: video_resolution, video_encoder_type ('clip...' selects the CLIP mean / std, anything
    else ImageNet's). antialias=False is the tensor Resize of the torchvision of the reference's era; True matches torchvision >= 0.17."""

    def __init__(self, opts, video_transforms="none", training=False, device="cuda", generator=None, antialias=False):
        super().__init__(device, training, generator)
        self.resolution = int(_opt(opts, "video_resolution", 224))
        clip = str(_opt(opts, "video_encoder_type", "clip")).startswith("clip")
        self.mean, self.std = (CLIP_MEAN, CLIP_STD) if clip else (IMAGENET_MEAN, IMAGENET_STD)
        if video_transforms not in ("none", "crop_flip"):
            raise NotImplementedError(video_transforms)
        if self.resolution <= 0:
            raise ValueError("video_resolution must be positive")
        self.video_transforms, self.antialias = video_transforms, bool(antialias)

    def geometry(self, clips):
        """int32 [F, 11]: one row per frame; the box and the flip of a clip are drawn once and shared by its frames"""
        rows = []
        for frames in clips:
            shapes = {tuple(f.shape) for f in frames}
            for f in frames:
                if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
                    raise ValueError("a frame is a uint8 array [H, W, 3]")
            if len(shapes) == 1:
                H, W, _ = next(iter(shapes))
                row = frame_geometry(H, W, self.resolution, self.video_transforms, self.training, self.generator)
                check_geometry(row, self.resolution)
                rows += [row] * len(frames)
            else:                                # frames of one clip that differ in size: a box each
                for f in frames:
                    row = frame_geometry(f.shape[0], f.shape[1], self.resolution, self.video_transforms, self.training, self.generator)
                    check_geometry(row, self.resolution)
                    rows.append(row)
        return np.asarray(rows, dtype=np.int32).reshape(len(rows), len(GEOM_FIELDS))

    def __call__(self, clips, stream=None, geometry=None):
        """clips: per clip a list of n uint8 [H, W, 3] arrays -> video_pixels fp32 [B, n, 3, R, R] on the device"""
        from . import kernels as K
        self._need_gpu()
        clips = [[f.numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in frames] for frames in clips]
        n = len(clips[0]) if clips else 0
        if n == 0 or any(len(c) != n for c in clips):
            raise ValueError("every clip needs the same, non-zero number of frames")
        geom = self.geometry(clips) if geometry is None else np.ascontiguousarray(geometry, dtype=np.int32)
        flat = [f for c in clips for f in c]
        if geom.shape != (len(flat), len(GEOM_FIELDS)):
            raise ValueError("geometry: one row of 11 per frame")
        for row, f in zip(geom.tolist(), flat):
            if (row[0], row[1]) != f.shape[:2]:
                raise ValueError("geometry: stored size differs from the frame")
            check_geometry(row, self.resolution)
        offsets = np.zeros(len(flat), dtype=np.int64)
        np.cumsum([f.size for f in flat[:-1]], out=offsets[1:])
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            d_off, d_geom, d_pix = _pack(self._ring, [offsets, geom, _Region(np.uint8, flat)], self.device, s)
            out = K.frames_prepare(d_pix, d_off, d_geom.view(geom.shape), self.resolution, self.mean, self.std, self.antialias)
        return out.view(len(clips), n, 3, self.resolution, self.resolution)


class BatchPrep:
    """AudioPrep + VideoPrep behind one call: prepare_batch(raw) adds `video_pixels` / `audio_spectrograms` to a batch dict."""

    def __init__(self, opts, video_transforms="none", training=False, device="cuda", generator=None, antialias=False, audio_sample_num=None):
        self.video = VideoPrep(opts, video_transforms, training, device, generator, antialias)
        self.audio = AudioPrep(opts, audio_sample_num, training, device, generator)
        self.device = self.video.device

    def prepare_batch(self, raw, stream=None, wait=True):
        """raw: {"frames": [per clip a list of uint8 HWC arrays], "wave": [per clip a 1-D array or None], "sample_rate": 16000, ...}.
        Returns a copy of `raw` without those three keys and with `video_pixels` / `audio_spectrograms` (device tensors) for the
        modalities present: one packed pinned host-to-device copy and one launch per modality, queued on `stream` (default: the
        current stream). With a side stream and wait=True the current stream is made to wait for it (the host is not blocked) and the
        tensors are recorded on it; wait=False leaves both to the caller (PrefetchLoader-style hand-over one step later)."""
        out = {k: v for k, v in raw.items() if k not in ("frames", "wave", "sample_rate")}
        made = []
        if raw.get("frames") is not None:
            out["video_pixels"] = self.video(raw["frames"], stream=stream)
            made.append(out["video_pixels"])
        if raw.get("wave") is not None:
            out["audio_spectrograms"] = self.audio(raw["wave"], sr=int(raw.get("sample_rate", 16000)), stream=stream)
            made.append(out["audio_spectrograms"])
        if stream is not None and wait:
            cur = torch.cuda.current_stream(self.device)
            if cur != stream:
                cur.wait_stream(stream)
                for t in made:
                    t.record_stream(cur)
        return out
