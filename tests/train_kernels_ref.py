"""Plain fp64 restatements of the training step's row, reduction and gradient-assembly kernels (train_kernels.hip), each with a DERIVED
per-element error bound, an fp32 emulation in a different summation order with switchable deliberate defects, and the seeded inputs
that tests/test_train_kernels_ref_cpu.py (CPU) and tests/test_train_rowkernels_gpu.py (GPU) share.  Nothing is tuned to a measured error.

Terms of every bound
====================
u32 = 2^-24 (fp32 unit roundoff), gam(n) = n u32 / (1 - n u32): the standard bound on n chained fp32 roundings in any order.
  * a sum of fp32 terms:        gam(p) * sum |terms|, p = the number of roundings on the longest path of the kernel's (fixed) reduction
                                order, one per addition plus one per multiply / divide applied to a term or to the result; every p below
                                is read off the kernel source and stated next to the function.  A fused multiply-add only removes a rounding.
  * one fp32 multiply / divide: u32 relative.
  * a bf16 output:              half a bf16 ulp OF the fp32 value that is rounded (round to nearest even).  For |v| in [2^e, 2^(e+1)) that
                                is 2^(e-8): between 2^-9 |v| (top of the binade) and 2^-8 |v| (a value just above a power of two, e.g.
                                1 + 2^-8 -> 1), so a flat 2^-9 |v| would refuse correctly rounded values; half_ulp_bf16 is the exact,
                                tightest form.  With a propagated error E on the fp32 value: E + half_ulp_bf16(|v| + E).
  * rsqrtf:                     2^-22 relative (documented 1 ulp = 2^-23, doubled as tests/attention_ref.py does for v_exp_f32).
  * (mean, rstd) from the slice partials (row_mean_rstd): with S = sum of the slice sums, Q = sum of the slice sums of squares,
        mean = S / D,  var = max(Q / D - mean^2, 0),  rstd = (var + eps)^-1/2
    the fp32 errors are propagated explicitly (mean_rstd below): e_var ~ u32 (c1 Q/D + c2 mean^2), so the relative error of var + eps is
    u32 * c * (Q/D + mean^2) / (var + eps): the cancellation factor comes out of the derivation and is returned for inspection.  The
    clamp is 1-Lipschitz and the exact variance is >= 0 up to the errors of the given partials, so it costs nothing.  rstd: the interval
    [W - e_w, W + e_w] of var + eps is pushed through x^-1/2 exactly (the lower end gives the larger error); e_w >= W would make the bound
    infinite -- the input families keep e_w far below W, and the CPU test asserts that every bound is finite.
  * 2^-100 * scale is added where a subnormal could appear.
Pure row moves and fp32 -> fp32 copies are compared bit for bit, bf16 copies against the correctly rounded value, bit for bit.
"""
import zlib

import torch

U32 = 2.0 ** -24
EPS_RSQ = 2.0 ** -22
TINY = 2.0 ** -100
LN_EPS = 1e-5
ROW_FAMILIES = ("benign", "scaled", "offset", "outlier", "constant")
ROW_D = (128, 384, 1280)
ROW_ROWS = (1, 5, 37)
OFFSET = 200.0                                       # the common offset of the "offset" family (row standard deviation 1)


def gam(n):
    return n * U32 / (1.0 - n * U32)


def f32(x):
    """the value a float argument has after the C ABI narrowed it to fp32"""
    return float(torch.tensor(x, dtype=torch.float32))


def half_ulp_bf16(a):
    """half a bf16 ulp at magnitude a >= 0 (fp64 tensor): 2^(e - 8) for a in [2^e, 2^(e+1))"""
    _, ex = torch.frexp(a.clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a), ex - 9)


def bf16_out(v, E):
    """bound on |bf16(v') - v| when |v' - v| <= E"""
    return E + half_ulp_bf16(v.abs() + E) + TINY


def bf16_round(x32):
    """correctly rounded bf16 of an fp32 tensor"""
    assert x32.dtype == torch.float32
    return x32.to(torch.bfloat16)


def rsqrt_err(W, e_w):
    """R = W^-1/2 and a bound on |rsqrtf(W') - R| for |W' - W| <= e_w (inf where e_w >= W)"""
    R = W.rsqrt()
    lo = W - e_w
    R_lo = torch.where(lo > 0, lo.clamp_min(1e-300).rsqrt(), torch.full_like(W, float("inf")))
    return R, (R_lo - R) + EPS_RSQ * R_lo


def gen(name, *key):
    return torch.Generator().manual_seed(zlib.crc32(("train_kernels/" + name + "/" + "/".join(str(k) for k in key)).encode()))


def assert_within(got, ref, bound, what, quiet=False):
    """every element finite and within its bound; returns (and prints) the worst error / bound ratio"""
    got = got.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert bool(torch.isfinite(bound).all()), f"{what}: the bound is not finite (this input tests nothing)"
    ratio = float(((got - ref).abs() / bound).max()) if got.numel() else 0.0
    if not quiet:
        print(f"{what}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error exceeds the derived bound, worst ratio {ratio:.3f}"
    return ratio


def breaches(got, ref, bound):
    """True when `got` (a defective result) leaves the bound somewhere (or is not finite, or has another shape)"""
    if got.shape != ref.shape:
        return True
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return True
    return bool(((got - ref).abs() > bound).any())


def bits_equal(a, b):
    """bit-for-bit equality of two tensors of the same dtype (NaN payloads included)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


# ---- inputs of the row kernels ----------------------------------------------------------------------------------------------------
def row_family(name, rows, D, tag="x"):
    """[rows, D] fp32.  benign: N(0, 1).  scaled: per-row magnitudes 2^-6 .. 2^6.  offset: N(0, 1) + (OFFSET + row % 7), sign alternating
    by row.  outlier: one channel of magnitude ~100 per row.  constant: every row a constant 0.3 + 0.1 (row % 5) (var = 0, clamped) except,
    with more than one row, the odd rows, which stay benign."""
    g = gen("row/" + name + "/" + tag, rows, D)
    x = torch.randn(rows, D, generator=g)
    r = torch.arange(rows, dtype=torch.float32)[:, None]
    if name == "benign":
        pass
    elif name == "scaled":
        ex = torch.linspace(-6.0, 6.0, rows)[torch.randperm(rows, generator=g)][:, None] if rows > 1 else torch.full((1, 1), -6.0)
        x = x * torch.exp2(ex)
    elif name == "offset":
        x = x + (OFFSET + r % 7) * (1 - 2 * (r % 2))
    elif name == "outlier":
        ch = (torch.arange(rows) * 37 + 5) % D
        x[torch.arange(rows), ch] = 100.0 * (1 - 2 * (torch.arange(rows) % 2).float()) * (1 + 0.01 * torch.arange(rows).float())
    elif name == "constant":
        c = (0.3 + 0.1 * (r % 5)).expand(rows, D)
        x = torch.where((r % 2 == 0).expand(rows, D), c, x)
    else:
        raise KeyError(name)
    return x.contiguous()


# ---- hb_stats: hb = bf16(H); stats[row][s] = (sum, sum of squares) over columns 64 s .. 64 s + 63 of the ROUNDED values ---------------
# a lane adds its two values (1), the 32 lanes of a half wave are added by 5 butterfly steps: p = 6; a square is one more rounding: 7
def hb_stats_ref(H):
    rows, D = H.shape
    hb = bf16_round(H)
    v = hb.double().view(rows, D // 64, 64)
    S, Q = v.sum(-1), (v * v).sum(-1)
    ref = torch.stack([S, Q], -1)
    bound = torch.stack([gam(6) * v.abs().sum(-1), gam(7) * Q], -1) + TINY
    return hb, ref, bound


def hb_stats_emul(H, defect=None):
    rows, D = H.shape
    hb = bf16_round(H)
    v = (H if defect == "stats_unrounded" else hb.float()).view(rows, D // 64, 64)
    st = torch.stack([v.sum(-1), (v * v).sum(-1)], -1)
    if defect == "slices_swapped":
        st = st.view(rows, D // 128, 2, 2).flip(2).reshape(rows, D // 64, 2)
    return hb, st


HB_STATS_DEFECTS = ("slices_swapped", "stats_unrounded")


# ---- row_mean_rstd ------------------------------------------------------------------------------------------------------------------
def mean_rstd(S, Q, eS, eQ, D, eps):
    """S, Q [rows, D/64] fp64: the slice sums the kernel is given (exact values), eS / eQ: what the GIVEN fp32 partials may be off by.
    wave_sum over the <= 20 partials (other lanes add exact zeros): 6 additions.  Returns mean, rstd, their error bounds [rows, 1] and
    the cancellation factor (Q/D + mean^2) / (var + eps)."""
    SM, SQ = S.sum(1, keepdim=True), Q.sum(1, keepdim=True)
    e_sm = eS.sum(1, keepdim=True) + gam(6) * (S.abs().sum(1, keepdim=True) + eS.sum(1, keepdim=True))
    e_sq = eQ.sum(1, keepdim=True) + gam(6) * (Q.abs().sum(1, keepdim=True) + eQ.sum(1, keepdim=True))
    M = SM / D
    e_m = e_sm / D + U32 * (M.abs() + e_sm / D)                                  # the division
    A = SQ / D
    e_a = e_sq / D + U32 * (A.abs() + e_sq / D)
    e_b = 2 * M.abs() * e_m + e_m ** 2 + U32 * (M.abs() + e_m) ** 2              # mean * mean
    V = A - M * M
    e_v = e_a + e_b + U32 * (V.abs() + e_a + e_b)                                # the subtraction; then max(., 0): 1-Lipschitz
    W = V.clamp_min(0) + eps
    e_w = e_v + U32 * (W + e_v)                                                  # + eps
    R, e_r = rsqrt_err(W, e_w)
    return M, R, e_m, e_r, (A + M * M) / W


def _xhat(xd, M, R, e_m, e_r):
    """x_hat = (x - mean) * rstd of exact x and the bound on the kernel's fp32 value"""
    c = xd - M
    e_c = e_m + U32 * (c.abs() + e_m)
    xh = c * R
    E = c.abs() * e_r + e_c * (R + e_r)
    return xh, E + U32 * (xh.abs() + E)


def _mean_rstd_f32(st, D, eps, defect=None):
    s = st[:, :-1] if defect == "last_slice_dropped" else st
    sm, sq = s[..., 0].sum(1, keepdim=True), s[..., 1].sum(1, keepdim=True)
    mean = sm / D
    var = (sq / D - mean * mean).clamp_min(0)
    return mean, torch.rsqrt(var + (0.0 if defect == "no_eps" else torch.tensor(eps, dtype=torch.float32)))


# ---- normalize: out = bf16((x - mean) * rstd), (mean, rstd) from caller-supplied stats ------------------------------------------------
def normalize_ref(x, stats, eps=LN_EPS):
    """x [rows, D] bf16, stats [rows, D/64, 2] fp32 (taken as exact inputs).  Returns x_hat, bound, (rstd, e_rstd, cancellation)"""
    rows, D = x.shape
    z = torch.zeros(rows, D // 64, dtype=torch.float64)
    M, R, e_m, e_r, cancel = mean_rstd(stats[..., 0].double(), stats[..., 1].double(), z, z, D, f32(eps))
    xh, E = _xhat(x.double(), M, R, e_m, e_r)
    return xh, bf16_out(xh, E), (R, e_r, cancel)


def normalize_emul(x, stats, eps=LN_EPS, defect=None):
    rows, D = x.shape
    st = stats.roll(-1, 0) if defect == "neighbour_stats" else stats
    mean, rstd = _mean_rstd_f32(st, D, eps, defect)
    return ((x.float() - mean) * rstd).to(torch.bfloat16)


NORMALIZE_DEFECTS = ("last_slice_dropped", "no_eps", "neighbour_stats")


# ---- ln_bwd (through ch_debug_ln_bwd: statistics by hb_stats from the bf16 x, then the row kernel) ------------------------------------
# per lane: s1 += g.x + g.y -> 2 additions per pass, 6 butterfly steps: p = 2 D/128 + 6, + the division; s2: + the product
def ln_bwd_ref(dyg, x, dres, eps=LN_EPS):
    """result = dres + rstd (dyg - mean(dyg) - x_hat mean(dyg x_hat)); returns (d, bound_d, x_hat, bound of the bf16 x_hat, (R, e_r, cancel))"""
    rows, D = x.shape
    xd, g = x.double(), dyg.double()
    v = xd.view(rows, D // 64, 64)
    S, Q = v.sum(-1), (v * v).sum(-1)
    M, R, e_m, e_r, cancel = mean_rstd(S, Q, gam(6) * v.abs().sum(-1), gam(7) * Q, D, f32(eps))
    xh, e_xh = _xhat(xd, M, R, e_m, e_r)
    p = 2 * (D // 128) + 6
    s1 = g.sum(1, keepdim=True) / D
    e_s1 = gam(p + 1) * g.abs().sum(1, keepdim=True) / D
    s2 = (g * xh).sum(1, keepdim=True) / D
    e_s2 = (gam(p + 2) * (g.abs() * (xh.abs() + e_xh)).sum(1, keepdim=True) + (g.abs() * e_xh).sum(1, keepdim=True)) / D
    t = g - s1 - xh * s2
    e_t = e_s1 + xh.abs() * e_s2 + e_xh * s2.abs() + e_xh * e_s2
    e_t = e_t + gam(3) * (g.abs() + s1.abs() + (xh * s2).abs() + e_t)
    rt = R * t
    e_rt = e_t * (R + e_r) + t.abs() * e_r
    e_rt = e_rt + U32 * (rt.abs() + e_rt)
    d = dres.double() + rt
    e_d = e_rt + U32 * (d.abs() + e_rt) + TINY
    return d, e_d, xh, bf16_out(xh, e_xh), (R, e_r, cancel)


def ln_bwd_emul(dyg, x, dres, eps=LN_EPS, defect=None):
    rows, D = x.shape
    xf, g = x.float(), dyg.float()
    _, st = hb_stats_emul(xf)
    mean, rstd = _mean_rstd_f32(st, D, eps, defect)
    xh = (xf - mean) * rstd
    s1 = g.sum(1, keepdim=True) / D
    s2 = (g * xh).sum(1, keepdim=True) / D
    if defect == "no_s1":
        s1 = s1 * 0
    if defect == "no_s2":
        s2 = s2 * 0
    return dres + rstd * (g - s1 - xh * s2), xh.to(torch.bfloat16)


LN_BWD_DEFECTS = ("last_slice_dropped", "no_s1", "no_s2")


# ---- LayerNorm backward from fp32 rows with the statistics computed in the kernel (embed_bwd, small_ln_bwd) --------------------------
def _ln_rows_core(x, dy, gamma, p, eps):
    """x, dy [rows, D], gamma [D] fp64 (exact inputs); p = additions on the longest path of one row reduction.
    Returns x_hat, dy o x_hat, dx and the bounds of the last two (fp32 outputs)."""
    D = x.shape[1]
    M = x.mean(1, keepdim=True)
    e_m = gam(p + 1) * x.abs().sum(1, keepdim=True) / D
    c = x - M
    e_c = e_m + U32 * (c.abs() + e_m)
    A = (c * c).mean(1, keepdim=True)
    e_sq = gam(p + 1) * ((c.abs() + e_c) ** 2).sum(1, keepdim=True) + (2 * c.abs() * e_c + e_c ** 2).sum(1, keepdim=True)
    e_a = e_sq / D + U32 * (A + e_sq / D)
    W = A + eps
    R, e_r = rsqrt_err(W, e_a + U32 * (W + e_a))
    xh = c * R
    e_xh = c.abs() * e_r + e_c * (R + e_r)
    e_xh = e_xh + U32 * (xh.abs() + e_xh)
    yx = dy * xh
    e_yx = dy.abs() * e_xh + U32 * (yx.abs() + dy.abs() * e_xh) + TINY
    g = dy * gamma
    e_g = U32 * g.abs()
    s1 = g.mean(1, keepdim=True)
    e_s1 = (gam(p + 1) * (g.abs() + e_g).sum(1, keepdim=True) + e_g.sum(1, keepdim=True)) / D
    s2 = (g * xh).mean(1, keepdim=True)
    e_s2 = (gam(p + 2) * ((g.abs() + e_g) * (xh.abs() + e_xh)).sum(1, keepdim=True)
            + (g.abs() * e_xh + e_g * xh.abs() + e_g * e_xh).sum(1, keepdim=True)) / D
    t = g - s1 - xh * s2
    e_t = e_g + e_s1 + xh.abs() * e_s2 + e_xh * s2.abs() + e_xh * e_s2
    e_t = e_t + gam(3) * (g.abs() + s1.abs() + (xh * s2).abs() + e_t)
    d = R * t
    e_d = e_t * (R + e_r) + t.abs() * e_r
    e_d = e_d + U32 * (d.abs() + e_d) + TINY
    return xh, yx, e_yx, d, e_d


def _ln_rows_f32(x, dy, gamma, eps, gamma_in_sums=True):
    D = x.shape[1]
    mean = x.sum(1, keepdim=True) / D
    c = x - mean
    rstd = torch.rsqrt((c * c).sum(1, keepdim=True) / D + torch.tensor(eps, dtype=torch.float32))
    xh = c * rstd
    g = dy * gamma
    gs = g if gamma_in_sums else dy
    s1 = gs.sum(1, keepdim=True) / D
    s2 = (gs * xh).sum(1, keepdim=True) / D
    return dy * xh, rstd * (g - s1 - xh * s2)


def ln_rows_autograd(x, dy, gamma):
    """fp64 autograd of y = LayerNorm(x) o gamma against the cotangent dy: (dx, dgamma)"""
    xd = x.double().clone().requires_grad_(True)
    gm = gamma.double().clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xd, (x.shape[1],), gm, None, f32(LN_EPS))
    y.backward(dy.double())
    return xd.grad, gm.grad


# ---- small_ln_bwd: one block of 256 threads per row: ceil(D / 256) serial additions, 8 tree steps ----------------------------------
SMALL_LN_SHAPES = tuple((r, D) for r in (1, 4) for D in (128, 384, 1000))
SMALL_LN_FAMILIES = ("benign", "offset", "scaled")


def small_ln_bwd_ref(dy, x, gamma, eps=LN_EPS):
    D = x.shape[1]
    _, _, _, d, e_d = _ln_rows_core(x.double(), dy.double(), gamma.double(), (D + 255) // 256 + 8, f32(eps))
    return d, e_d


def small_ln_bwd_emul(dy, x, gamma, eps=LN_EPS, defect=None):
    if defect == "x_uncentred":
        D = x.shape[1]
        rstd = torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + eps)
        g = dy * gamma
        xh = x * rstd
        return rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return _ln_rows_f32(x, dy, gamma, eps, gamma_in_sums=defect != "no_gamma_in_sums")[1]


SMALL_LN_DEFECTS = ("no_gamma_in_sums", "x_uncentred")


def small_ln_inputs(rows, D, family):
    g = gen("small_ln", rows, D, family)
    return torch.randn(rows, D, generator=g), row_family(family, rows, D, "small_ln"), 1 + 0.3 * torch.randn(D, generator=g)


# ---- embed_bwd --------------------------------------------------------------------------------------------------------------------
# one wave per row: 2 additions per pass and lane, 6 butterfly steps: p = 2 D/128 + 6
EMBED_SHAPES = tuple((2, np_, Q, D) for (np_, Q) in ((4, 1), (49, 4)) for D in ROW_D)


def embed_inputs(B, np_, Q, D, family):
    """X [B * ntok, D] (patch rows valid, CLS / concept rows NaN: the kernel takes those from cls_pos0 / ctx), dY, cls_pos0, ctx, gamma"""
    ntok = 1 + np_ + Q
    g = gen("embed", B, np_, Q, D, family)
    X = row_family(family, B * ntok, D, "embed")
    t = torch.arange(B * ntok) % ntok
    X[(t == 0) | (t > np_)] = float("nan")
    dY = torch.randn(B * ntok, D, generator=g)
    cls = row_family(family, 1, D, "cls")[0] * 0.5
    ctx = row_family(family, Q + 2, D, "ctx")[2:] * 1.5
    gamma = 1 + 0.3 * torch.randn(D, generator=g)
    return X, dY, cls, ctx, gamma


def embed_source_rows(X, ntok, np_, cls, ctx, defect=None):
    """the pre-LayerNorm input rows the kernel normalises"""
    rows = X.shape[0]
    Q = ntok - np_ - 1
    t = torch.arange(rows) % ntok
    src = X.clone()
    if defect != "cls_from_x":
        src[t == 0] = cls
    qi = (t - np_ - 1)[t > np_]
    if defect == "concept_off_by_one":
        qi = (qi + 1) % Q
    src[t > np_] = ctx[qi]
    return src


def embed_bwd_ref(X, dY, B, ntok, np_, cls, ctx, gamma, eps=LN_EPS):
    """(X_out, bound, dY_out, bound, compact patch rows (exact value), bound of their bf16 form)"""
    D = X.shape[1]
    src = embed_source_rows(X, ntok, np_, cls, ctx).double()
    _, yx, e_yx, d, e_d = _ln_rows_core(src, dY.double(), gamma.double(), 2 * (D // 128) + 6, f32(eps))
    t = torch.arange(B * ntok) % ntok
    patch = (t >= 1) & (t <= np_)
    return yx, e_yx, d, e_d, d[patch], bf16_out(d[patch], e_d[patch])


def embed_bwd_emul(X, dY, B, ntok, np_, cls, ctx, gamma, eps=LN_EPS, defect=None):
    src = embed_source_rows(X, ntok, np_, cls, ctx, defect)
    yx, d = _ln_rows_f32(src, dY, gamma, eps, gamma_in_sums=defect != "no_gamma_in_sums")
    rows = B * ntok
    t = torch.arange(rows) % ntok
    img = torch.arange(rows) // ntok
    patch = (t >= 1) & (t <= np_)
    dxp = torch.zeros(B * np_, X.shape[1], dtype=torch.bfloat16)
    stride = ntok if defect == "compact_ntok" else np_
    idx = img[patch] * stride + t[patch] - 1
    keep = idx < B * np_                                  # (the defective index would run past the compact array: dropped here)
    dxp[idx[keep]] = d[patch][keep].to(torch.bfloat16)
    return yx, d, dxp


EMBED_DEFECTS = ("concept_off_by_one", "cls_from_x", "compact_ntok", "no_gamma_in_sums")


# ---- colsum: out[n] = sum_m A[m][n] over two stages ---------------------------------------------------------------------------------
COLSUM_ROWS = (1, 7, 8, 255, 257, 1000, 32801)
COLSUM_N = (8, 128, 264, 384)


def colsum_cases():
    """(rows, N, lda, family): every row count with every N except the largest with the small N only; one lda > N; one cancelling input"""
    cases = [(r, n, n, "benign") for r in COLSUM_ROWS[:-1] for n in COLSUM_N]
    cases += [(COLSUM_ROWS[-1], 8, 8, "benign"), (COLSUM_ROWS[-1], 8, 8, "cancel"), (257, 264, 272, "benign"), (1000, 128, 128, "cancel")]
    return cases


def colsum_launch(rows):
    chunks = min(128, (rows + 255) // 256)
    return chunks, (rows + chunks - 1) // chunks


def colsum_paths(rows):
    """roundings on the longest path: a row lane owns n = ceil(chunk_rows / 8) rows; whole groups of four go one each to the four
    accumulators, the n % 4 rows left over all go to accumulator 0 (the tail loop), so its chain is floor(n / 4) + n % 4 additions (the
    first, to 0, is exact but counted); 2 to combine the accumulators, 7 across the row lanes; reduce_partials: ceil(chunks / 8) per chunk
    lane, 7 across"""
    chunks, cr = colsum_launch(rows)
    n = (cr + 7) // 8
    return n // 4 + n % 4 + 2 + 7 + (chunks + 7) // 8 + 7


def colsum_input(rows, N, lda, family, is_f32):
    g = gen("colsum", rows, N, lda, family, is_f32)
    a = torch.randn(rows, lda, generator=g)
    if family == "cancel":                                 # true column sums nearly cancel: row r + 1 = -row r (+ 2^-10 noise)
        h = rows // 2
        a[h:2 * h] = -a[:h] + 2.0 ** -10 * torch.randn(h, lda, generator=g)
    return a if is_f32 else a.to(torch.bfloat16)


def colsum_ref(A, N):
    a = A[:, :N].double()
    return a.sum(0), gam(colsum_paths(A.shape[0])) * a.abs().sum(0) + TINY


def colsum_emul(A, N, defect=None):
    rows = A.shape[0]
    chunks, cr = colsum_launch(rows)
    a = A[:, :N].float()
    if defect == "halves_swapped" and A.dtype == torch.bfloat16:
        a = a.view(rows, N // 2, 2).flip(2).reshape(rows, N)
    out = torch.zeros(N)
    for c in range(chunks):
        if defect == "chunk_skipped" and c == chunks // 2:
            continue
        r0, r1 = c * cr, min(rows, (c + 1) * cr)
        if defect == "tail_group_dropped":
            r1 = r0 + (r1 - r0 - 1) // 8 * 8                 # the last group of (up to) 8 rows of the chunk
        out = out + a[r0:r1].sum(0)
    return out


COLSUM_DEFECTS = ("tail_group_dropped", "chunk_skipped", "halves_swapped")


# ---- reduce_partials_multi: out[i] = sum_c partial[c][i]; chunk lane l adds chunks l, l + 8, ..., the 8 lanes are added in order -----
REDUCE_CASES = ((1, (1,), (1,)), (1, (7,), (33,)), (1, (128,), (32,)), (2, (8, 9), (31, 33)), (2, (64, 1), (32, 1)),
                (4, (1, 7, 9, 128), (32, 31, 33, 1)), (4, (8, 64, 128, 7), (33, 32, 1, 31)))       # (njobs, nchunks, n4)


def reduce_input(j, nchunks, n4):
    return torch.randn(nchunks, 4 * n4, generator=gen("reduce", j, nchunks, n4))


def reduce_ref(partial):
    p = partial.double()
    return p.sum(0), gam((partial.shape[0] + 7) // 8 + 7) * p.abs().sum(0) + TINY


def reduce_multi_emul(partials, defect=None):
    outs = []
    for j, p in enumerate(partials):
        if defect == "first_eight_chunks_only":
            p = p[:8]
        if defect == "last_chunk_dropped":
            p = p[:-1]
        o = p.flip(0).sum(0)
        if defect == "last_block_dropped" and o.numel() > 128:
            o = o.clone()
            o[(o.numel() - 1) // 128 * 128:] = 0
        outs.append(o)
    return outs


REDUCE_DEFECTS = ("last_chunk_dropped", "last_block_dropped", "first_eight_chunks_only")


# ---- transposes: dst[c][r] = bf16(src[r][c] * colscale[c]) -- one fp32 product, one rounding: bit for bit ------------------------------
TRANSPOSE_SHAPES = ((1, 1), (31, 33), (32, 32), (200, 384), (384, 200))
TRANSPOSE_DEFECTS = ("scale_by_row", "tile_not_transposed", "ld_src_ignored")


def transpose_input(R, C, ld_src, is_f32):
    g = gen("transpose", R, C, ld_src, is_f32)
    src = torch.randn(R, ld_src, generator=g)
    return (src if is_f32 else src.to(torch.bfloat16)), 1 + 0.3 * torch.randn(C, generator=g)


def transpose_ref(src, C, colscale=None, defect=None):
    """defects (emulation only): scale_by_row, tile_not_transposed (square shapes), ld_src_ignored (rows read C apart, not ld_src)"""
    v = src[:, :C].float()
    if defect == "ld_src_ignored":
        v = src.reshape(-1)[:src.shape[0] * C].view(src.shape[0], C).float()
    if colscale is not None:
        v = v * (colscale[:v.shape[0], None] if defect == "scale_by_row" and v.shape[0] <= C else colscale[None, :])
    if defect == "tile_not_transposed" and v.shape[0] == v.shape[1]:
        return v.to(torch.bfloat16).contiguous()
    return v.t().to(torch.bfloat16).contiguous()


# ---- adapter arena --------------------------------------------------------------------------------------------------------------------
ADAPTER_SHAPES = ((128, 8), (384, 200), (768, 384))          # (D, b): bpad 128, 256, 384
ADAPTER_NAD = (1, 3)


def adapter_numel(D, b):
    return 2 * D + b * D + b + D * b + D + 1


def bpad_of(b):
    return (b + 127) // 128 * 128


def adapter_fields(blk, D, b):
    """views of one adapter's block: ln_w, ln_b, down_w [b, D], down_b, up_w [D, b], up_b, scale"""
    o = [0, D, 2 * D, 2 * D + b * D, 2 * D + b * D + b, 2 * D + b * D + b + D * b, 2 * D + b * D + b + D * b + D]
    return (blk[o[0]:o[1]], blk[o[1]:o[2]], blk[o[2]:o[3]].view(b, D), blk[o[3]:o[4]], blk[o[4]:o[5]].view(D, b), blk[o[5]:o[6]],
            blk[o[6]:o[6] + 1])


def adapter_arena(D, b, nad, stride):
    g = gen("arena", D, b, nad, stride)
    P = torch.randn(nad * stride, generator=g)
    for a in range(nad):
        ln_w, ln_b, dw, db, uw, ub, sc = adapter_fields(P[a * stride:], D, b)
        ln_w.mul_(0.3).add_(1.0)
        ln_b.mul_(0.5)
        dw.mul_(D ** -0.5)
        uw.mul_(b ** -0.5)
        sc.fill_(0.6 + 0.3 * a)
    return P


def adapter_refresh_ref(P, stride, nad, D, b):
    """per adapter: Wdf [bpad, D] bf16 (exact), c, d (+ bounds) [bpad], up_w [D, bpad] bf16, up_wT [b, D] bf16, down_wgT [D, b] bf16 -- the
    two transposed copies carry only the rows / columns the kernel writes"""
    bp = bpad_of(b)
    out = []
    for a in range(nad):
        ln_w, ln_b, dw, db, uw, ub, _ = adapter_fields(P[a * stride:], D, b)
        wdf = torch.zeros(bp, D, dtype=torch.bfloat16)
        wdf[:b] = (dw * ln_w[None, :]).to(torch.bfloat16)
        p = D // 64 + (D % 64 != 0) + 6                     # a lane's serial additions + 6 butterfly steps
        c = wdf.double().sum(1)
        e_c = gam(p) * wdf.double().abs().sum(1) + TINY
        d = torch.zeros(bp, dtype=torch.float64)
        d[:b] = db.double() + (dw.double() * ln_b.double()[None, :]).sum(1)
        e_d = torch.full((bp,), TINY, dtype=torch.float64)
        e_d[:b] += gam(p + 2) * (db.double().abs() + (dw.double() * ln_b.double()[None, :]).abs().sum(1))
        up = torch.zeros(D, bp, dtype=torch.bfloat16)
        up[:, :b] = uw.to(torch.bfloat16)
        out.append(dict(wdf=wdf, c=c, e_c=e_c, d=d, e_d=e_d, up=up, upT=uw.t().to(torch.bfloat16).contiguous(),
                        dwgT=(dw * ln_w[None, :]).t().to(torch.bfloat16).contiguous()))
    return out


def adapter_refresh_emul(P, stride, nad, D, b, defect=None):
    bp = bpad_of(b)
    out = []
    for a in range(nad):
        ln_w, ln_b, dw, db, uw, ub, _ = adapter_fields(P[a * stride:], D, b)
        prod = dw * ln_w[None, :]
        wdf = torch.zeros(bp, D, dtype=torch.bfloat16)
        wdf[:b] = prod.to(torch.bfloat16)
        c = torch.zeros(bp)
        c[:b] = (prod if defect == "c_unrounded" else wdf[:b].float()).flip(1).sum(1)
        d = torch.zeros(bp)
        d[:b] = db + (0 if defect == "d_without_beta" else (dw * ln_b[None, :]).flip(1).sum(1))
        up = torch.zeros(D, bp, dtype=torch.bfloat16)
        up[:, :b] = uw.to(torch.bfloat16)
        if defect == "padding_not_zero" and bp > b:
            wdf[b] = wdf[b - 1]
            up[:, b] = up[:, b - 1]
            c[b], d[b] = c[b - 1], d[b - 1]
        out.append(dict(wdf=wdf, c=c, d=d, up=up, upT=uw.t().to(torch.bfloat16).contiguous(), dwgT=prod.t().to(torch.bfloat16).contiguous()))
    return out


REFRESH_DEFECTS = ("c_unrounded", "d_without_beta", "padding_not_zero")


def adapter_grad_operands(P, stride, nad, D, b):
    """G [nad, D, bpad], cu [nad, D], T [nad, bpad, D], cd [nad, bpad]: columns / rows past b hold NaN (never read), and G, cu are correlated
    with up_w, up_b so that <G, W_up> and <cu, b_up> are both far above the summation error and of comparable size"""
    bp = bpad_of(b)
    g = gen("adapter_grads", D, b, nad, stride)
    G = torch.full((nad, D, bp), float("nan"))
    T = torch.full((nad, bp, D), float("nan"))
    cu = torch.randn(nad, D, generator=g)
    cd = torch.full((nad, bp), float("nan"))
    for a in range(nad):
        _, _, dw, _, uw, ub, _ = adapter_fields(P[a * stride:], D, b)
        G[a, :, :b] = torch.randn(D, b, generator=g) * b ** -0.5 + uw * (0.5 + 0.1 * a)          # <G, W_up> ~ 0.5 D
        cu[a] = cu[a] + ub * (0.4 + 0.1 * a)                                                       # <cu, b_up> ~ 0.4 D
        T[a, :b] = torch.randn(b, D, generator=g) + dw * D ** 0.5
        cd[a, :b] = torch.randn(b, generator=g)
    return G, cu, T, cd


def adapter_grads_ref(G, cu, T, cd, P, stride, nad, D, b):
    """gradient arena blocks [nad, adapter_numel] fp64 and their bounds.  d(scale): a thread adds ceil(D b / 65536) + ceil(D / 65536)
    products, two 8-step trees; dgamma / dbeta: ceil(b / 64) products per lane, 64 lane sums added in order"""
    n = adapter_numel(D, b)
    ref = torch.zeros(nad, n, dtype=torch.float64)
    bound = torch.zeros(nad, n, dtype=torch.float64)
    p_s = -(-D * b // 65536) + -(-D // 65536) + 8 + 8 + 1
    p_k = -(-b // 64) + 64 + 1
    for a in range(nad):
        ln_w, ln_b, dw, _, uw, ub, sc = (f.double() for f in adapter_fields(P[a * stride:], D, b))
        Ga, Ta, cda, cua = G[a, :, :b].double(), T[a, :b].double(), cd[a, :b].double(), cu[a].double()
        s = sc[0]
        r_lnw, r_lnb, r_dw, r_db, r_uw, r_ub, r_s = adapter_fields(ref[a], D, b)
        e_lnw, e_lnb, e_dw, e_db, e_uw, e_ub, e_s = adapter_fields(bound[a], D, b)
        r_dw.copy_(Ta * ln_w[None, :] + cda[:, None] * ln_b[None, :])
        e_dw.copy_(gam(2) * ((Ta * ln_w[None, :]).abs() + (cda[:, None] * ln_b[None, :]).abs()))
        r_db.copy_(cda)                                                                            # a copy: exact
        r_uw.copy_(s * Ga)
        e_uw.copy_(U32 * (s * Ga).abs())
        r_ub.copy_(s * cua)
        e_ub.copy_(U32 * (s * cua).abs())
        r_s.copy_(((Ga * uw).sum() + (cua * ub).sum()).view(1))
        e_s.copy_((gam(p_s) * ((Ga * uw).abs().sum() + (cua * ub).abs().sum())).view(1))
        r_lnw.copy_((Ta * dw).sum(0))
        e_lnw.copy_(gam(p_k) * (Ta * dw).abs().sum(0))
        r_lnb.copy_((cda[:, None] * dw).sum(0))
        e_lnb.copy_(gam(p_k) * (cda[:, None] * dw).abs().sum(0))
    return ref, bound + TINY


def adapter_grads_emul(G, cu, T, cd, P, stride, nad, D, b, defect=None):
    n = adapter_numel(D, b)
    bp = bpad_of(b)
    out = torch.zeros(nad, n)
    for a in range(nad):
        slot = 0 if (defect == "slot_of_adapter_0" and a == 1) else a
        ln_w, ln_b, dw, _, uw, ub, sc = adapter_fields(P[a * stride:], D, b)
        Ga = G[slot, :, :b]
        if defect == "G_ld_b":
            Ga = G[slot].reshape(-1)[:D * b].view(D, b)
        Ta, cda, cua = T[slot, :b], cd[slot, :b], cu[slot]
        o_lnw, o_lnb, o_dw, o_db, o_uw, o_ub, o_s = adapter_fields(out[a], D, b)
        o_dw.copy_(Ta * ln_w[None, :] + cda[:, None] * ln_b[None, :])
        o_db.copy_(cda)
        o_uw.copy_(Ga if defect == "dW_up_unscaled" else sc[0] * Ga)
        o_ub.copy_(sc[0] * cua)
        ds = (Ga * uw).flip(0).sum()
        if defect != "ds_without_cu_bup":
            ds = ds + (cua * ub).sum()
        o_s.copy_(ds.view(1))
        o_lnw.copy_((Ta * dw).flip(0).sum(0))
        o_lnb.copy_(((Ta if defect == "dbeta_from_T" else cda[:, None]) * dw).flip(0).sum(0))
    return out


ADAPTER_GRADS_DEFECTS = ("ds_without_cu_bup", "dbeta_from_T", "G_ld_b", "slot_of_adapter_0", "dW_up_unscaled")


def adapter_grads_autograd(dH, x_hat, dpre, g_act, P_blk, D, b):
    """fp64 autograd of the adapter's parameters for a batch: pre = W_dn (gamma o x_hat + beta) + b_dn with cotangent dpre, and
    out = s (g W_up^T + b_up) with cotangent dH (g held fixed: the activation between the two has its own kernel)"""
    ln_w, ln_b, dw, db, uw, ub, sc = (f.double().clone().requires_grad_(True) for f in adapter_fields(P_blk, D, b))
    pre = (x_hat * ln_w + ln_b) @ dw.t() + db
    out = sc * (g_act @ uw.t() + ub)
    ((pre * dpre).sum() + (out * dH).sum()).backward()
    return torch.cat([ln_w.grad, ln_b.grad, dw.grad.reshape(-1), db.grad, uw.grad.reshape(-1), ub.grad, sc.grad])


# ---- fold_grads ---------------------------------------------------------------------------------------------------------------------
FOLD_SHAPES = tuple((D, nparts, re) for D in (128, 384) for (nparts, re) in ((1, 1), (1, 200), (3, 65), (3, 128)))


def fold_inputs(D, nparts, rows_each):
    g = gen("fold", D, nparts, rows_each)
    n = nparts * rows_each
    W = [torch.randn(rows_each, D, generator=g) * D ** -0.5 for _ in range(nparts)]
    T = torch.randn(n, D, generator=g) + torch.cat(W) * D ** 0.5
    c = torch.randn(n, generator=g) * (1 + torch.arange(n) // rows_each)
    return T, c, 1 + 0.3 * torch.randn(D, generator=g), 0.5 * torch.randn(D, generator=g), W


def fold_grads_ref(T, c, gamma, beta, W):
    """(dW [n, D], bound, db [n] (exact copy), dgamma, bound, dbeta, bound); a row lane adds nparts * ceil(rows_each / 64) products, then 64"""
    Td, cd, Wd = T.double(), c.double(), torch.cat(W).double()
    a1, a2 = Td * gamma.double()[None, :], cd[:, None] * beta.double()[None, :]
    p = len(W) * -(-W[0].shape[0] // 64) + 64 + 1
    return (a1 + a2, gam(2) * (a1.abs() + a2.abs()) + TINY, cd, (Td * Wd).sum(0), gam(p) * (Td * Wd).abs().sum(0) + TINY,
            (cd[:, None] * Wd).sum(0), gam(p) * (cd[:, None] * Wd).abs().sum(0) + TINY)


def fold_grads_emul(T, c, gamma, beta, W, defect=None):
    """returns (dW [n, D], db [n], dgamma, dbeta) with the parts' outputs concatenated in part order"""
    nparts, re = len(W), W[0].shape[0]
    Wc = torch.cat(W)
    dW = T * gamma[None, :] + (0 if defect == "dW_without_c_beta" else c[:, None] * beta[None, :])
    db = c.clone()
    if defect == "parts_rotated" and nparts > 1:
        dW, db = dW.roll(re, 0), db.roll(re, 0)
    if defect == "db_part0_only":
        db[re:] = 0
    rows = slice(0, re) if defect == "dgamma_part0_only" else slice(0, nparts * re)
    return dW, db, (T[rows] * Wc[rows]).flip(0).sum(0), ((T if defect == "dbeta_from_T" else c[:, None]) * Wc).flip(0).sum(0)


FOLD_DEFECTS = ("parts_rotated", "db_part0_only", "dgamma_part0_only", "dW_without_c_beta", "dbeta_from_T")


def fold_grads_autograd(x_hat, dpre, gamma, beta, W):
    """fp64 autograd of pre = W (gamma o x_hat + beta) + b: (dW, db, dgamma, dbeta)"""
    gm, bt = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    Wd = torch.cat(W).double().clone().requires_grad_(True)
    bias = torch.zeros(Wd.shape[0], dtype=torch.float64, requires_grad=True)
    pre = (x_hat * gm + bt) @ Wd.t() + bias
    (pre * dpre).sum().backward()
    return Wd.grad, bias.grad, gm.grad, bt.grad


# ---- row moves and row sums of the concept tokens ------------------------------------------------------------------------------------------
MOVE_SHAPES = tuple((3, 21, Q, D) for Q in (1, 4) for D in (128, 384))
MOVE_DEFECTS = ("concept_block_early", "concept_block_late")


def _con0(ntok, Q, defect):
    return ntok - Q + {None: 0, "concept_block_early": -1, "concept_block_late": 1}[defect]


def token_rows_sum_ref(dX, B, ntok, nrows):
    v = dX.double().view(B, ntok, -1)[:, :nrows]
    return v.sum(0), gam(B) * v.abs().sum(0) + TINY


def concept_rows_sum_ref(dH, B, ntok, Q):
    v = dH.double().view(B, ntok, -1)[:, ntok - Q:]
    return v.sum(0), gam(B) * v.abs().sum(0) + TINY


def concept_rows_sum_emul(dH, B, ntok, Q, defect=None):
    c0 = _con0(ntok, Q, defect)
    rows = (torch.arange(B)[:, None] * ntok + c0 + torch.arange(Q)[None, :]).clamp_max(B * ntok - 1)
    return dH[rows].flip(0).sum(0)


def token_rows_sum_emul(dX, B, ntok, nrows, defect=None):
    off = {None: 0, "concept_block_early": -1, "concept_block_late": 1}[defect]
    rows = (torch.arange(B)[:, None] * ntok + off + torch.arange(nrows)[None, :]).clamp(0, B * ntok - 1)
    return dX[rows].flip(0).sum(0)


def scatter_concept_rows_ref(dhf, B, ntok, Q):
    """(dH fp32, dHb bf16): exact"""
    D = dhf.shape[-1]
    dH = torch.zeros(B, ntok, D)
    dH[:, ntok - Q:] = dhf.view(B, Q, D)
    dH = dH.view(B * ntok, D)
    return dH, dH.to(torch.bfloat16)


def expand_head_rows_ref(src, B, ntok, Q):
    """src [B * (1 + Q), D] (slot 0 = CLS, 1.. = concept tokens) -> [B * ntok, D], zero elsewhere: exact, either dtype"""
    D = src.shape[-1]
    dst = torch.zeros(B, ntok, D, dtype=src.dtype)
    s = src.view(B, 1 + Q, D)
    dst[:, ntok - Q:] = s[:, 1:]
    dst[:, 0] = s[:, 0]
    return dst.view(B * ntok, D)


def gather_concept_rows_ref(H, B, ntok, Q):
    return H.view(B, ntok, -1)[:, ntok - Q:].reshape(B * Q, -1).contiguous()


def row_move_emul(kind, src, B, ntok, Q, defect=None):
    """the three moves written as the kernels are, one destination row at a time with its own index arithmetic (not the slicing of the
    restatements above); `defect` moves the first concept row.  kind: scatter | expand | gather"""
    c0 = _con0(ntok, Q, defect)
    D = src.shape[-1]
    if kind == "gather":
        out = torch.zeros(B * Q, D, dtype=src.dtype)
        for r in range(B * Q):
            out[r] = src[min((r // Q) * ntok + c0 + r % Q, B * ntok - 1)]
        return out
    out = torch.zeros(B * ntok, D, dtype=src.dtype)
    for row in range(B * ntok):
        t, img = row % ntok, row // ntok
        if kind == "scatter" and c0 <= t < c0 + Q:
            out[row] = src[img * Q + t - c0]
        if kind == "expand" and (t == 0 or c0 <= t < c0 + Q):
            out[row] = src[img * (1 + Q) + (0 if t == 0 else 1 + t - c0)]
    return out
