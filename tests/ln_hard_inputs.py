"""Hard rows for the fused bias + dropout + residual + LayerNorm kernels (valor_amd/csrc/layernorm.hip), the fp64 references they are held
against, element-wise bounds, and one judge (a plain host module like attn_hard_inputs.py and dropout_ref.py; no GPU code).

Row classes cycle with the row index (class = (row + rows) % 7: the last four rows of 37 hold classes 0-3, those of 333 classes 4-6 and 0,
so between the two row counts every class meets the ragged last workgroup of every family). Every value
is exact in the storage type. The class shapes the LAST operand of the sum -- `residual` when the form has one, else `x`; the other
operands are N(0, 0.25^2):
  benign         N(0, 1)
  offset         fp32: 1000 + 0.01 N(0, 1); bf16: 64 + N(0, 1), rounded            |mean| >> sigma
  outlier        N(0, 1) with +300 in column 1 and -180 in column cols - 2         the first and the last lane's vectors
  tiny           2^-10 N(0, 1): variance ~1e-6, eps = 1e-5 decides rstd             pins where eps enters
  big            2^15 N(0, 1)
  near-constant  5.0 everywhere, one element 5 + 2^-5
  constant       3.25
Backward dy classes cycle at period 4: benign, one-hot (one non-zero per row), constant 1.0 (with gamma = 1 the exact LN' is 0: pure
cancellation), 2^10 N(0, 1). gamma = 1 + N(0, 1) with columns 0, 5, cols - 1 set to 0 and columns 2, cols - 3 negative; beta = N(0, 1).

References, all in fp64 from the rounded inputs:
  z               dropout_ref.ref_bdrln_dropout's law (keep mask of dropout_ref.ln_keep, dropout_ref.keep_scale, the row scale)
  y, mean, rstd   from the z THE KERNEL STORED (the statistics are defined on the stored value, layernorm.hip's header), from the input sum
                  when z is not written. eps is the fp32 value the kernel receives.
  backward        z, mean, rstd are INPUTS of valor_bdrln_bwd: xh = (z - mean) rstd with the given fp32 mean / rstd,
                  dz = rstd (gy - mean_j gy - xh mean_j(gy xh)) + dz_in, gy = dy gamma; dx = dz keep keep_scale row_scale;
                  dgamma, dbeta, dbias = column sums of dy xh, dy, dx. Independent of the forward: z may be any rows.

Bounds, element-wise, from the arithmetic. U32 = 2^-24; U(dtype) = 2^-9 for a bf16 output, 0 for fp32; S(ref) = U(dtype) 2^ceil(log2 |ref|),
one store of the result (amendment (i)); Z_r = max_j |z_rj|:
  z       nops U32 sum|operand terms| + S(ref)     nops = one per fp32 operation that formed it: + bias, dropout 3 (amendment (ii)),
                                                   * row_scale, + residual
  mean    8 U32 Z_r
  rstd    relative 16 (U32 + d_r^2), d_r = U32 Z_r rstd_r        d_r^2: how far a mean that is off by its own bound moves the variance
  y       8 U32 (Z_r rstd_r |gamma_j| + |y_ref| + |beta_j|) + S(y_ref)
  dres    8 U32 (rstd_r (|gy_rj| + mean_j|gy| + |xh_rj| mean_j|gy xh|) + |dz_ref| + |dz_in|) + S(ref)
  dx      the fp32 part of the dres bound times the multiplier keep_scale |row_scale| that carries it into dx, + U32 |ref| when dropout or a
          row scale multiplies, + S(ref)
  dgamma / dbeta / dbias, per column      (D + 3) U32 sum_r|term_rj| + S(ref); dbias: + sum_r of the fp32 part of the dx bound (amendment (iv));
          into a sink: + U32 |prior + ref| (amendment (iii)) + S(prior + ref)
The constants 8 and 16: an fp32 emulation of the kernels' summation order (per-lane sequential adds, then a butterfly over the lane group;
tests/test_ln_hard_inputs_cpu.py restates it) stayed within 2.1 x the unit-constant form of the mean, y and dz expressions and within 5.0 x
for rstd over all seven classes, both eps and the width / lane-group pairs 100/64, 128/16, 192/8, 768/64, 768/32, 1024/32, 2048/64, 4096/256.

Amendments. The first statement of these bounds had U(dtype) |ref| for every store, nops = 1 for the dropout, no fp32 term for the accumulate
and no term for what a dbias addend carries in. The plain fp32 restatement AND the MI355X kernels both landed above 1.0 in exactly these four
places and nowhere else, by the same factors; each is a term the arithmetic has and the expression lacked (no constant was changed):
  (i)   a store to bf16 rounds to 8 significant bits: the result moves by up to half an ulp of its binade [2^e, 2^(e+1)), 2^(e-8) = U 2^(e+1),
        which is U |ref| only at the top of the binade and 2 U |ref| at its bottom. With U |ref| every bf16-stored output of the restatement and
        of every kernel sat at 1.8-2.0 (1 + 2^-8 + 2^-20 stores as 1 + 2^-7); with S(ref) at 0.96-1.00.
  (ii)  the kernels multiply by the fp32 keep_scale 1.0f / (1.0f - p): two more fp32 operations (0.77 U32 off dropout_ref.keep_scale at p = 0.1,
        0.50 U32 at p = 0.25) before the multiply. Counted as one, fp32 z sat at 1.00-1.12 (full form, 3 operations) and 1.27-1.33 (2 operations:
        no bias / no residual) on the kernels, 1.04 in the restatement; p = 0 stayed at 0.95.
  (iii) `out = prior + sum` is an fp32 addition also when the output is fp32 (U(dtype) = 0): valor_colsum with accumulate, 1 row of 3070 fp32
        columns, sat at 5.4 where |x_j| << |prior_j|.
  (iv)  the addends of dbias are the dx values, each off by up to the fp32 part of its own bound (the LN' cancellation: with rstd = 1e6 on a
        constant row under eps = 1e-12 and dy = 2^10 N(0, 1), every dx of the row moves with the rounding of mean_j(gy)), not by 3 roundings of
        itself: the fp32 plain LayerNorm at 768 columns, 37 rows sat at 1.51 in one column. dgamma's and dbeta's addends are products of inputs.

D, the longest chain of fp32 additions one addend of a column sum passes through, read off layernorm.hip. colsum_finalize{,3}: 1024 partial
rows, thread (ry, cx) adds rows ry + 16 j + 256 it into s_(j % 4): 4 iterations x 4 adds = 16, then (s0 + s1) + (s2 + s3) = 2, then the
16-step loop over red[][cx] = 16: FIN = 34. With G(n) = ceil(rows / n) trips round the 1024-workgroup grid-stride loop:
  wave      ln_bwd_kernel: one row per wave and trip, G(4096) adds in the lane's register, 4 in the cross-wave loop:    D = G(4096) + 4 + FIN
  half      ln_bwd_h_kernel<NV8, GL>: RPW = 64 / GL rows per wave and trip, 4 RPW lane groups cross:        D = G(4096 RPW) + 4 RPW + FIN
  lds       ln_bwd_h_kernel<3, 32, true>: both half-waves add to one LDS array, then (a + b) + (c + d):        D = 2 G(8192) + 2 + FIN
  wide      ln_bwd_wide_kernel: one row per workgroup and trip, every column has one owner:                         D = G(1024) + FIN
  colsum    colsum_partial_kernel: one row per wave and trip, then r0 + r1 + r2 + r3:                            D = G(4096) + 3 + FIN

judge(name, got, ref, bound) compares element by element, NaN / Inf in `got` is a failure; on failure it reports the count, the first flat
index, its row class and its column. judge_all() runs it over every output of a launch, prints one `PARITY ln ...` line with the largest
observed / allowed ratio per output, and only then raises."""
import types

import numpy as np
import torch

import dropout_ref as R

BF16, F32 = torch.bfloat16, torch.float32
CLASSES = ("benign", "offset", "outlier", "tiny", "big", "near-constant", "constant")
BENIGN, OFFSET, OUTLIER, TINY, BIG, NEARCONST, CONST = range(7)
DY_CLASSES = ("benign", "one-hot", "ones", "big")
U32 = 2.0 ** -24
U_BF16 = 2.0 ** -9
C_MEAN, C_RSTD, C_Y, C_DZ, C_TERM = 8, 16, 8, 8, 3
PART_BLOCKS, FWD_BLOCKS_CAP, FIN_DEPTH = 1024, 8192, 34


def store_term(ref, dtype):
    """what one round-to-nearest store of `ref` in `dtype` may add to the fp32 arithmetic: U(dtype) times the power of two that closes ref's
    binade, half a bf16 ulp there (amendment (i) of the module docstring); nothing for fp32"""
    a = ref.double().abs()
    if dtype != BF16:
        return torch.zeros_like(a)
    m, e = torch.frexp(a)                                   # a = m 2^e, m in [0.5, 1)
    top = torch.ldexp(torch.ones_like(a), e)
    return U_BF16 * torch.where(a > 0, torch.where(m == 0.5, top / 2, top), torch.zeros_like(a))


def row_classes(rows, device="cpu"):
    """class of every row: the cycle's phase is the row count, so the last four rows of 37 hold classes 0-3 and those of 333 classes 4-6, 0"""
    return (torch.arange(rows, device=device) + rows) % len(CLASSES)


# ---------------------------------------------------------------------------------------------- inputs
def _randn(shape, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(shape, generator=g, device=device, dtype=F32)


def hard_rows(rows, cols, dtype, seed, device="cpu", hard=True):
    """[rows, cols] in the storage type; hard=False: benign rows only"""
    n = _randn((rows, cols), seed, device)
    if not hard:
        return n.to(dtype)
    cls = row_classes(rows, device)[:, None]
    r = torch.arange(rows, device=device)
    nb = n.to(dtype).float()                                   # rounded first: the power-of-two scalings below stay exact
    ol = n.clone(); ol[:, 1] = 300.0; ol[:, cols - 2] = -180.0
    nc = torch.full_like(n, 5.0); nc[r, (7 * r + 3) % cols] = 5.0 + 2.0 ** -5
    out = torch.where(cls == OFFSET, (1000.0 + 0.01 * n) if dtype == F32 else (64.0 + n), n)
    out = torch.where(cls == OUTLIER, ol, out)
    out = torch.where(cls == TINY, nb * 2.0 ** -10, out)
    out = torch.where(cls == BIG, nb * 2.0 ** 15, out)
    out = torch.where(cls == NEARCONST, nc, out)
    out = torch.where(cls == CONST, torch.full_like(n, 3.25), out)
    return out.to(dtype)


def small(shape, dtype, seed, device="cpu"):
    return (0.25 * _randn(shape, seed, device)).to(dtype)


def make_gamma(cols, dtype, seed, device="cpu"):
    g = 1.0 + _randn((cols,), seed, device)
    g[[2, cols - 3]] = -(g[[2, cols - 3]].abs() + 0.5)
    g[[0, 5, cols - 1]] = 0.0
    return g.to(dtype)


def make_dy(rows, cols, dtype, seed, device="cpu", hard=True):
    n = _randn((rows, cols), seed, device)
    if not hard:
        return n.to(dtype)
    cls = (torch.arange(rows, device=device) % len(DY_CLASSES))[:, None]
    r = torch.arange(rows, device=device)
    hot = torch.zeros_like(n); hot[r, (11 * r + 1) % cols] = 3.0
    out = torch.where(cls == 1, hot, n)
    out = torch.where(cls == 2, torch.ones_like(n), out)
    out = torch.where(cls == 3, n.to(dtype).float() * 2.0 ** 10, out)
    return out.to(dtype)


def make_case(rows, cols, dtype, seed=0, device="cpu", hard=True, bias=True, residual=True, gamma=True, beta=True, dy=True, dz_in=True):
    """operands of one form; absent ones are None. The class rows are the last operand of the sum."""
    shaped = hard_rows(rows, cols, dtype, seed + 1, device, hard)
    c = types.SimpleNamespace(rows=rows, cols=cols, dtype=dtype, cls=row_classes(rows, device) if hard else None)
    c.x = small((rows, cols), dtype, seed + 2, device) if residual else shaped
    c.residual = shaped if residual else None
    c.bias = small((cols,), dtype, seed + 3, device) if bias else None
    c.gamma = make_gamma(cols, dtype, seed + 4, device) if gamma else None
    c.beta = _randn((cols,), seed + 5, device).to(dtype) if beta else None
    c.dy = make_dy(rows, cols, dtype, seed + 6, device, hard) if dy else None
    c.dz_in = small((rows, cols), dtype, seed + 7, device) if dz_in else None
    return c


def keep_mask(seed, offset, rows, cols, p, device="cpu"):
    return torch.from_numpy(R.ln_keep(seed, offset, rows, cols, p)).to(device) if p > 0 else None


def _row_factor(row_scale, rows_per_scale, rows, device):
    if row_scale is None:
        return None
    return row_scale.double()[torch.arange(rows, device=device) // rows_per_scale][:, None]


# ---------------------------------------------------------------------------------------------- references and bounds
def ref_z(x, bias, residual, keep, p, row_scale, rows_per_scale, dtype):
    """fp64 z and its bound"""
    t = x.double(); a = t.abs(); nops = 0
    if bias is not None:
        t = t + bias.double(); a = a + bias.double().abs(); nops += 1
    if keep is not None:
        k = keep.double() * R.keep_scale(p)
        t = t * k; a = a * k; nops += 3                     # 1.0f - p, 1.0f / that, and the multiply: amendment (ii)
    f = _row_factor(row_scale, rows_per_scale, x.shape[0], x.device)
    if f is not None:
        t = t * f; a = a * f.abs(); nops += 1
    if residual is not None:
        t = t + residual.double(); a = a + residual.double().abs(); nops += 1
    return t, nops * U32 * a + store_term(t, dtype)


def ref_stats(z, eps):
    """fp64 mean / rstd of the rows of z (the stored z, or the fp64 sum when none is stored) with their bounds, and Z_r"""
    zd = z.double()
    mean = zd.mean(-1)
    var = ((zd - mean[:, None]) ** 2).mean(-1)
    rstd = (var + float(np.float32(eps))) ** -0.5
    zmax = zd.abs().amax(-1)
    d = U32 * zmax * rstd
    return mean, rstd, C_MEAN * U32 * zmax, C_RSTD * (U32 + d * d) * rstd, zmax


def ref_y(z, mean, rstd, zmax, gamma, beta, dtype):
    y = (z.double() - mean[:, None]) * rstd[:, None]
    g = torch.ones_like(y[0]) if gamma is None else gamma.double()
    b = torch.zeros_like(y[0]) if beta is None else beta.double()
    y = y * g + b
    return y, C_Y * U32 * ((zmax * rstd)[:, None] * g.abs() + y.abs() + b.abs()) + store_term(y, dtype)


def forward_items(c, got, eps, keep=None, p=0.0, row_scale=None, rows_per_scale=0):
    """(name, got, ref, bound) of every output the forward returned; got = (z, y, mean, rstd) of kernels.bdrln_fwd"""
    z, y, mean, rstd = got
    zr, zb = ref_z(c.x, c.bias, c.residual, keep, p, row_scale, rows_per_scale, c.dtype)
    items = [("z", z, zr, zb)] if z is not None else []
    if y is not None:
        mr, rr, mb, rb, zmax = ref_stats(z if z is not None else zr, eps)
        yr, yb = ref_y(z if z is not None else zr, mr, rr, zmax, c.gamma, c.beta, c.dtype)
        items += [("y", y, yr, yb), ("mean", mean, mr, mb), ("rstd", rstd, rr, rb)]
    return items


def colsum_depth(family, rows, gl=32):
    G = lambda n: -(-rows // n)
    if family == "wave":
        return G(4096) + 4 + FIN_DEPTH
    if family == "half":
        rpw = 64 // gl
        return G(4096 * rpw) + 4 * rpw + FIN_DEPTH
    if family == "lds":
        return 2 * G(8192) + 2 + FIN_DEPTH
    if family == "wide":
        return G(1024) + FIN_DEPTH
    assert family == "colsum", family
    return G(4096) + 3 + FIN_DEPTH


def ln_group(cols):
    """lanes per row of the 16-byte-access kernels (layernorm.hip ln_group), 0: not covered"""
    if cols % 256 == 0 and cols <= 1024:
        return 32
    return 16 if cols in (128, 384) else 8 if cols == 192 else 0


def bwd_depth(rows, cols, dtype, variant, aligned=True, has_dy=True, has_dz_in=True):
    """D of the backward family launch_ln_bwd picks"""
    gl = ln_group(cols)
    lacc = variant == 1 and cols == 768 and rows >= 49152 and has_dy and has_dz_in
    if dtype == BF16 and variant >= 1 and gl and aligned and (variant >= 2 or lacc or cols == 1024 or cols <= 256):
        if cols == 768 and (variant == 3 or lacc):
            return colsum_depth("lds", rows)
        return colsum_depth("half", rows, gl)
    return colsum_depth("wide" if cols > 2048 else "wave", rows)


def colsum_bound(terms_abs_sum, ref, depth, dtype, prior=None, term_err=None):
    """term_err: sum over the rows of the error each addend may carry in beyond C_TERM roundings of itself (amendment (iv))"""
    b = (depth + C_TERM) * U32 * terms_abs_sum + store_term(ref, dtype)
    if term_err is not None:
        b = b + term_err
    if prior is not None:
        total = prior.double() + ref
        b = b + U32 * total.abs() + store_term(total, dtype)          # the fp32 add onto the prior (amendment (iii)) and its store
    return b


def backward_items(c, z, mean, rstd, got, depth, keep=None, p=0.0, row_scale=None, rows_per_scale=0, priors=(None, None, None)):
    """(name, got, ref, bound) of every output the backward returned; got = (dx, dres, dgamma, dbeta, dbias) of kernels.bdrln_bwd, with the
    sink tensors in the slots of `got` where sinks= was used and their prior contents in `priors`"""
    dx, dres, dg, db, dbias = got
    dt = c.dtype
    ref = c.dy if c.dy is not None else c.dz_in
    rows = ref.shape[0]
    dzi = torch.zeros_like(ref, dtype=torch.float64) if c.dz_in is None else c.dz_in.double()
    if c.dy is not None:
        rs = rstd.double()[:, None]
        xh = (z.double() - mean.double()[:, None]) * rs
        dyd = c.dy.double()
        gy = dyd if c.gamma is None else dyd * c.gamma.double()
        dz = rs * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True)) + dzi
        f32 = rs * (gy.abs() + gy.abs().mean(-1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(-1, keepdim=True))
    else:
        dz, f32 = dzi, torch.zeros_like(dzi)
    f32 = C_DZ * U32 * (f32 + dz.abs() + dzi.abs())
    mult = torch.ones_like(dz)
    if keep is not None:
        mult = mult * keep.double() * R.keep_scale(p)
    f = _row_factor(row_scale, rows_per_scale, rows, ref.device)
    if f is not None:
        mult = mult * f
    dxr = dz * mult
    items = [("dres", dres, dz, f32 + store_term(dz, dt))]
    scaled = keep is not None or f is not None
    dx32 = f32 * mult.abs() + (U32 if scaled else 0.0) * dxr.abs()
    items.append(("dx", dx, dxr, dx32 + store_term(dxr, dt)))
    for name, o, term, prior in (("dgamma", dg, None if c.dy is None else dyd * xh, priors[0]),
                                 ("dbeta", db, None if c.dy is None else dyd, priors[1]), ("dbias", dbias, dxr, priors[2])):
        if o is None:
            continue
        s = term.sum(0)
        bound = colsum_bound(term.abs().sum(0), s, depth, dt, prior, dx32.sum(0) if name == "dbias" else None)
        items.append((name, o, s if prior is None else s + prior.double(), bound))
    return items


# ---------------------------------------------------------------------------------------------- the judge
def judge(name, got, ref, bound, cls=None):
    """largest observed / allowed ratio; raises AssertionError when an element is off by more than its bound or is not finite"""
    g, r = got.double(), ref.double()
    b = torch.broadcast_to(bound.double(), r.shape)
    assert g.shape == r.shape, (name, tuple(g.shape), tuple(r.shape))
    err = (g - r).abs()
    bad = ~torch.isfinite(g) | ~(err <= b)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        name_of = lambda row: f"row {row}" + (f" ({CLASSES[int(cls[row])]})" if cls is not None else "")
        if g.dim() == 2:
            where = f"flat index {i}, {name_of(i // g.shape[1])}, column {i % g.shape[1]}"
        elif cls is not None and g.shape[0] == cls.shape[0]:          # mean / rstd: one value per row
            where = f"flat index {i}, {name_of(i)}"
        else:                                                          # a column sum
            where = f"flat index {i}, column {i}"
        raise JudgeError(f"{name}: {nbad} of {g.numel()} elements off, first at {where}: got {float(g.reshape(-1)[i])!r}, "
                         f"reference {float(r.reshape(-1)[i])!r}, allowed {float(b.reshape(-1)[i]):.3e}; largest observed/allowed {worst:.3g}", worst)
    return worst


class JudgeError(AssertionError):
    def __init__(self, msg, worst):
        super().__init__(msg)
        self.worst = worst


def judge_all(tag, items, cls=None):
    """judge every (name, got, ref, bound), print the ratios, then raise for all that failed; returns {name: ratio}"""
    ratios, failed = {}, []
    for name, got, ref, bound in items:
        try:
            ratios[name] = judge(name, got, ref, bound, cls)
        except JudgeError as e:
            ratios[name] = e.worst
            failed.append(str(e))
    print("PARITY ln hard", tag, {n: f"{v:.3f}" for n, v in ratios.items()}, "observed/allowed", flush=True)
    assert not failed, f"{tag}: " + " | ".join(failed)
    return ratios
