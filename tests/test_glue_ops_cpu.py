"""Argument checks of the small glue entry points (misc.hip, the two means, the smoothed cross-entropy), without a GPU: every call below
must come back from the host-side validation -- an empty problem is a no-op (0), a width the 4-wide kernels cannot take, an unknown
dtype or a null required pointer is VALOR_ERR_ARG (-1) -- and none of them may reach a kernel launch (a null pointer that got through
would be a GPU fault, not an error code)."""
import ctypes

import pytest

F = (ctypes.c_float * 256)()          # stands in for every data pointer: nothing here is ever dereferenced
I64 = (ctypes.c_int64 * 16)()
BAD_DT = 7

# name -> (good argument list, {index of every REQUIRED pointer}, (index, value) that makes the problem empty,
#          [(index, value) that must be refused], index of dtype or None)
# Each good list is a valid call (it is never made as it stands: it would launch).
CASES = {
    # (stream, dtype, in, out, N, C, H, W, P, ld_out)
    "valor_patchify": ([None, 1, F, F, 2, 3, 32, 48, 16, 768], {2, 3}, (4, 0),
                       [(8, 15), (6, 40), (7, 40), (9, 767), (8, 3)], 1),
    # (stream, dtype, in, frame_emb, type_emb, out, Bn, F, X, E, out_bs, out_row_off)
    "valor_add_frame_type_fwd": ([None, 1, F, F, F, F, 2, 3, 5, 8, 120, 0], {2, 3, 4, 5}, (6, 0), [(9, 6), (9, 2)], 1),
    # (stream, dtype, dout, din, dframe, part, Bn, F, X, E, out_bs, out_row_off)
    "valor_add_frame_type_bwd": ([None, 1, F, F, F, F, 2, 3, 5, 8, 120, 0], {2, 3, 4, 5}, (6, 0), [(9, 6), (9, 2)], 1),
    # (stream, dtype, x, y, norm, rows, cols)
    "valor_l2norm_fwd": ([None, 1, F, F, F, 4, 8], {2, 3, 4}, (5, 0), [(6, 6), (6, 1)], 1),
    # (stream, dtype, y, dy, norm, dx, rows, cols)
    "valor_l2norm_bwd": ([None, 1, F, F, F, F, 4, 8], {2, 3, 4, 5}, (6, 0), [(7, 6), (7, 1)], 1),
    # (stream, dtype, src, idx, out | dst, n, E, ld)
    "valor_gather_rows": ([None, 1, F, I64, F, 4, 8, 8], {2, 3, 4}, (5, 0), [(6, 6), (7, 10)], 1),
    "valor_scatter_rows": ([None, 1, F, I64, F, 4, 8, 8], {2, 3, 4}, (5, 0), [(6, 6), (7, 10)], 1),
    # (stream, dtype, x, w, b, y, rows, cols): b optional
    "valor_rowdot_fwd": ([None, 1, F, F, F, F, 4, 8], {2, 3, 5}, (6, 0), [(7, 6), (7, 3)], 1),
    # (stream, dtype, dy, x, w, dx, dw, db, rows, cols): db optional
    "valor_rowdot_bwd": ([None, 1, F, F, F, F, F, F, 4, 8], {2, 3, 4, 5, 6}, (8, 0), [(9, 6), (9, 3)], 1),
    # (stream, dtype, dh, u, du, n, act)
    "valor_dact_mul": ([None, 1, F, F, F, 16, 1], {2, 3, 4}, (5, 0), [(5, 6), (5, 17)], 1),
    # (stream, dtype, in, out, n)
    "valor_cast_from_f32": ([None, 1, F, F, 16], {2, 3}, (4, 0), [(4, 6), (4, 17)], 1),
    # (stream, dtype, in | dout, out | din, groups, X, E)
    "valor_group_mean_fwd": ([None, 1, F, F, 2, 3, 8], {2, 3}, (4, 0), [(6, 6), (5, 0)], 1),
    "valor_group_mean_bwd": ([None, 1, F, F, 2, 3, 8], {2, 3}, (4, 0), [(6, 6), (5, 0)], 1),
    # (stream, dtype, patches, cls, pos, bias, out, N, Pn, E): bias optional
    "valor_assemble_tokens_fwd": ([None, 1, F, F, F, F, F, 2, 3, 8], {2, 3, 4, 6}, (7, 0), [(9, 6)], 1),
    # (stream, dtype, dout, dpatches, dpos, dcls, N, Pn, E, accumulate): dcls optional
    "valor_assemble_tokens_bwd": ([None, 1, F, F, F, F, 2, 3, 8, 0], {2, 3, 4}, (6, 0), [(8, 6)], 1),
    # (stream, dtype, x, dsum, N, Tn, E, accumulate)
    "valor_sum_over_batch": ([None, 1, F, F, 2, 3, 8, 0], {2, 3}, (5, 0), [(6, 6)], 1),
    # (stream, dtype, ids, dout, dword, n, E, accumulate)
    "valor_embed_bwd_word": ([None, 1, I64, F, F, 4, 8, 0], {2, 3, 4}, (5, 0), [(6, 6)], 1),
}


@pytest.fixture(scope="module")
def so():
    from valor_amd import lib
    return lib.load()


def _with(args, i, v):
    a = list(args)
    a[i] = v
    return a


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_point_validates_before_launching(so, name):
    good, required, (ei, ev), refused, dti = CASES[name]
    fn = getattr(so, name)
    assert fn(*_with(good, ei, ev)) == 0, "an empty problem is a no-op"
    assert fn(*_with(good, ei, -1)) == 0, "a negative count is an empty problem too"
    for i, v in refused:
        assert fn(*_with(good, i, v)) == -1, (name, "argument", i, "=", v)
    for dt in (0, 1):                                        # both element types: the check sits in front of the dispatch
        for i in sorted(required):
            assert fn(*_with(_with(good, dti, dt), i, None)) == -1, (name, "null pointer at", i, "dtype", dt)
    assert fn(*_with(good, dti, BAD_DT)) == -1 and fn(*_with(good, dti, -1)) == -1, "unknown dtype"
    # an empty problem stays a no-op whatever the pointers are (callers pass null for tensors they did not allocate)
    assert fn(*[None if i in required else a for i, a in enumerate(_with(good, ei, ev))]) == 0


def test_patchify_geometry_is_checked(so):
    """odd P, H or W that P does not divide, ld_out < K, and the 2-wide path's even-W requirement"""
    good = CASES["valor_patchify"][0]
    call = lambda **kw: so.valor_patchify(*[kw.get(k, v) for k, v in zip(("st", "dt", "i", "o", "N", "C", "H", "W", "P", "ld"), good)])
    assert call(P=15, H=30, W=45, ld=675) == -1              # odd P although it divides H and W
    assert call(H=40) == -1 and call(W=40) == -1             # H % P, W % P
    assert call(ld=767) == -1                                # ld_out < K = 3 * 16 * 16
    assert call(P=14, H=28, W=42, ld=587) == -1              # ld_out < K = 588 on the 2-wide path
    assert call(N=0, P=15) == 0                              # empty comes first


def test_means_and_smoothed_xent_refuse_degenerate_sizes(so):
    assert so.valor_mean_f32(None, F, 0, F) == -1 and so.valor_mean_f32(None, F, -3, F) == -1
    assert so.valor_mean_f32(None, None, 4, F) == -1 and so.valor_mean_f32(None, F, 4, None) == -1
    assert so.valor_weighted_mean_f32(None, F, F, 0, F) == -1
    for args in ((None, F, 4, F), (F, None, 4, F), (F, F, 4, None)):
        assert so.valor_weighted_mean_f32(None, *args) == -1
    # label smoothing spreads eps over the V - 1 other classes: V = 1 has none
    assert so.valor_xent_smooth_fwd(None, 1, F, I64, F, F, 4, 1, 32, 0.1) == -1
    assert so.valor_xent_smooth_bwd(None, 1, F, I64, F, None, 1.0, 4, 1, 32, 0.1) == -1
    assert so.valor_xent_smooth_fwd(None, 1, F, I64, F, F, 0, 1, 32, 0.1) == 0          # no rows: no-op
    assert so.valor_xent_smooth_fwd(None, 1, F, I64, F, F, 4, 0, 32, 0.0) == -1         # V = 0
    assert so.valor_xent_smooth_fwd(None, 1, F, I64, F, F, 4, 16, 32, 1.0) == -1        # smoothing outside [0, 1)
    assert so.valor_xent_smooth_fwd(None, BAD_DT, F, I64, F, F, 4, 16, 32, 0.1) == -1
    assert so.valor_xent_fwd(None, 1, None, I64, F, F, 4, 16, 32) == -1
    assert so.valor_xent_bwd(None, 1, F, None, F, None, 1.0, 4, 16, 32) == -1
