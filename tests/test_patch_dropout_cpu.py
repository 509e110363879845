"""CPU: video patch dropout -- the host law of the subset draw (tests/patch_keep_ref.py), the option handling of the model's constructor
and the argument checks of the four entry points of valor_amd/csrc/patchdrop.hip (which return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import patch_keep_ref as PR


def test_host_law_rows_are_sorted_subsets_with_their_inverse():
    N, Pn, k = 6, 16, 5
    idx, slot = PR.patch_keep_host(1234, 77, N, Pn, k, 1)
    assert idx.shape == (N, k) and slot.shape == (N, Pn) and idx.dtype == np.int32 and slot.dtype == np.int32
    for f in range(N):
        row = idx[f]
        assert np.all(np.diff(row) > 0) and row[0] >= 0 and row[-1] < Pn            # sorted, distinct, in range: a k-subset
        assert np.array_equal(slot[f, row], np.arange(k))                           # slot inverts idx ...
        assert np.all(np.delete(slot[f], row) == -1)                                # ... and is -1 everywhere else
    assert len({tuple(r) for r in idx}) > 1                                         # different frames draw different subsets
    # the law itself on one frame: the k smallest keys of philox(seed, offset + f * Pn + p), written out with Python ints
    import dropout_ref as R
    f = 3
    keys = []
    for p in range(Pn):
        w = R.philox4x32_10_scalar(1234, 77 + f * Pn + p)
        keys.append((w[0] | (w[1] << 32), p))
    assert sorted(p for _, p in sorted(keys)[:k]) == list(idx[f])


def test_host_law_tube_rows_of_a_clip_are_equal_and_groups_differ():
    N, Pn, k, F = 8, 16, 8, 4
    idx, slot = PR.patch_keep_host(5, 0, N, Pn, k, F)
    for g in range(N // F):
        for f in range(g * F, (g + 1) * F):
            assert np.array_equal(idx[f], idx[g * F]) and np.array_equal(slot[f], slot[g * F])
    assert not np.array_equal(idx[0], idx[F])
    # group g of a tube draw uses the counters frame g of a per-frame draw uses
    per_frame, _ = PR.patch_keep_host(5, 0, N // F, Pn, k, 1)
    assert np.array_equal(idx[::F], per_frame)


def test_host_law_full_and_single():
    idx, slot = PR.patch_keep_host(9, 3, 2, 16, 16, 1)
    assert np.array_equal(idx, np.tile(np.arange(16, dtype=np.int32), (2, 1))) and np.array_equal(slot, idx)
    idx, slot = PR.patch_keep_host(9, 3, 3, 16, 1, 1)
    assert idx.shape == (3, 1) and np.all((slot >= 0).sum(1) == 1)


def test_keep_frequency_is_uniform():
    """n = 4096 frames, Pn = 16, k = 8: a patch is kept with probability 1/2, its frequency over n independent frames has standard
    deviation sqrt(0.25 / n); six of them = 0.047 (a 2e-9 event per patch under the law)."""
    n, Pn, k = 4096, 16, 8
    _, slot = PR.patch_keep_host(42, 1 << 20, n, Pn, k, 1)
    freq = (slot >= 0).mean(axis=0)
    bound = 6.0 * (0.25 / n) ** 0.5
    assert np.all(np.abs(freq - 0.5) <= bound), (freq, bound)


def test_kept_count_law():
    from valor_amd.model.valor import patch_keep_count
    assert patch_keep_count(196, 0.0) == 196                  # rate 0: nothing dropped
    assert patch_keep_count(196, 0.5) == 98 and patch_keep_count(196, 0.25) == 147 and patch_keep_count(196, 0.75) == 49
    assert patch_keep_count(16, 0.99) == 1 and patch_keep_count(1, 0.9) == 1            # never fewer than one patch
    assert patch_keep_count(196, 0.5, keep=95) == 95          # the exact count overrides the rate
    assert patch_keep_count(256, 0.3) == 256 - int(256 * 0.3)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            patch_keep_count(196, bad)
    for bad in (0, 197, -3):
        with pytest.raises(ValueError):
            patch_keep_count(196, 0.0, keep=bad)


def _model(opts, spec=None):
    from valor_amd import synth
    from valor_amd.model.valor import VALOR
    return VALOR(opts, spec=spec or synth.tiny_spec(), dtype=torch.float32, device="cpu")


def test_options_and_refusals():
    from valor_amd import synth
    m = _model({"video_patch_dropout": 0.5})
    assert (m.patch_keep, m.patch_dropout_mode) == (8, "frame") and m.last_patch_keep is None
    m = _model({"video_patch_dropout": 0.5, "video_patch_keep": 5, "video_patch_dropout_mode": "tube"})
    assert (m.patch_keep, m.patch_dropout_mode) == (5, "tube")
    # off: no option, rate 0, or every patch kept
    for opts in (None, {}, {"video_patch_dropout": 0.0}, {"video_patch_keep": 16}, {"video_patch_dropout": 0.01}):
        m = _model(opts)
        assert m.patch_keep is None and not m._patch_dropout_active()
    # active in training passes only
    m = _model({"video_patch_dropout": 0.5})
    assert m.train()._patch_dropout_active()
    with torch.no_grad():
        assert not m._patch_dropout_active()
    assert not m.eval()._patch_dropout_active()
    for opts in ({"video_patch_dropout": 1.0}, {"video_patch_dropout": -0.2}, {"video_patch_keep": 0}, {"video_patch_keep": 17},
                 {"video_patch_dropout": 0.5, "video_patch_dropout_mode": "block"}):
        with pytest.raises(ValueError):
            _model(opts)
    with pytest.raises(NotImplementedError, match="scst"):
        _model({"video_patch_dropout": 0.5, "scst_finetuning": True})
    with pytest.raises(NotImplementedError, match="VideoSwin"):
        _model({"video_patch_dropout": 0.5}, synth.tiny_swin_spec())
    with pytest.raises(NotImplementedError, match="VideoSwin"):
        _model({"video_patch_keep": 4}, synth.tiny_swin_spec())
    _model({"scst_finetuning": True})                         # ... and neither refusal fires without the option
    _model(None, synth.tiny_swin_spec())


def test_draw_counters_takes_exactly_n():
    from valor_amd.ops import DropoutState
    seed0, off0 = DropoutState.seed, DropoutState.offset
    try:
        DropoutState.reset(7, 100)
        assert DropoutState.draw_counters(48) == (7, 100) and DropoutState.offset == 148
        assert DropoutState.draw_counters(0) == (7, 148) and DropoutState.offset == 148
    finally:
        DropoutState.reset(seed0, off0)


def test_ops_refuse_bad_tables_before_any_launch():
    from valor_amd import ops
    with pytest.raises(ValueError):
        ops.patch_keep(6, 16, 8, group=4, device="cpu")       # N % group
    with pytest.raises(ValueError):
        ops.patch_keep(4, 16, 17, device="cpu")
    with pytest.raises(ValueError):
        ops.patch_keep(4, 16, 0, device="cpu")
    img = torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError):
        ops.patchify(img, 16, torch.float32, keep=torch.zeros(2, 2, dtype=torch.int64))       # not int32
    with pytest.raises(ValueError):
        ops.patchify(img, 16, torch.float32, keep=torch.zeros(3, 2, dtype=torch.int32))       # another N
    with pytest.raises(ValueError):
        ops.patchify(img, 16, torch.float32, keep=torch.zeros(2, 5, dtype=torch.int32))       # k > Pn = 4


def test_entry_points_validate_arguments_without_gpu():
    """the four entries return -1 on a bad argument before any launch; N = 0 frames is a no-op of the data-movement entries"""
    from valor_amd import lib
    so = lib.load()
    i32 = (ctypes.c_int32 * 256)()
    f32 = (ctypes.c_float * 4096)()

    def keep(N=4, Pn=16, k=8, group=1, idx=i32, slot=i32):
        return so.valor_patch_keep(None, N, Pn, k, group, 1, 0, None, idx, slot)

    assert keep(idx=None) == -1 and keep(slot=None) == -1
    assert keep(N=0) == -1 and keep(N=-2) == -1
    assert keep(Pn=0) == -1 and keep(Pn=1025, k=8) == -1
    assert keep(k=0) == -1 and keep(k=17) == -1
    assert keep(group=0) == -1 and keep(group=3) == -1 and keep(group=-1) == -1

    def patchify(dt=1, i=f32, idx=i32, o=f32, N=1, C=3, H=32, W=32, P=16, k=2, ld=768):
        return so.valor_patchify_kept(None, dt, i, idx, o, N, C, H, W, P, k, ld)

    assert patchify(i=None) == -1 and patchify(idx=None) == -1 and patchify(o=None) == -1
    assert patchify(dt=7) == -1
    assert patchify(k=0) == -1 and patchify(k=5) == -1                       # 4 patches per image
    assert patchify(P=15) == -1 and patchify(H=40) == -1 and patchify(W=40) == -1 and patchify(ld=700) == -1
    assert patchify(P=0) == -1 and patchify(C=0) == -1
    assert patchify(N=0) == 0

    def fwd(dt=1, pa=f32, cls=f32, pos=f32, bias=None, idx=i32, o=f32, N=2, Pn=4, k=2, E=8):
        return so.valor_assemble_tokens_kept_fwd(None, dt, pa, cls, pos, bias, idx, o, N, Pn, k, E)

    assert fwd(pa=None) == -1 and fwd(cls=None) == -1 and fwd(pos=None) == -1 and fwd(idx=None) == -1 and fwd(o=None) == -1
    assert fwd(dt=5) == -1 and fwd(E=6) == -1 and fwd(E=0) == -1
    assert fwd(k=0) == -1 and fwd(k=5) == -1 and fwd(Pn=0) == -1
    assert fwd(N=0) == 0

    def bwd(dt=1, do=f32, slot=i32, dp=f32, dpos=f32, dcls=None, N=2, Pn=4, k=2, E=8, acc=0):
        return so.valor_assemble_tokens_kept_bwd(None, dt, do, slot, dp, dpos, dcls, N, Pn, k, E, acc)

    assert bwd(do=None) == -1 and bwd(slot=None) == -1 and bwd(dp=None) == -1 and bwd(dpos=None) == -1
    assert bwd(dt=5) == -1 and bwd(E=6) == -1 and bwd(k=0) == -1 and bwd(k=5) == -1 and bwd(Pn=0) == -1
    assert bwd(N=0) == 0
