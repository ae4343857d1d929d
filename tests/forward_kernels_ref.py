"""Plain fp64 restatements of the forward row kernels (rowops.hip), the hashing head (head.hip) and the load-time folds (small_f32.hip), each
with a DERIVED per-element error bound, an fp32 emulation in a different summation order with switchable deliberate defects, and the seeded
inputs that tests/test_forward_kernels_ref_cpu.py (CPU) and tests/test_forward_kernels_gpu.py (GPU) share.  Nothing is tuned to a measured
error.  The vocabulary (u32, gam(p), half_ulp_bf16, bf16_out, rsqrt_err, TINY) is that of tests/train_kernels_ref.py; p, the number of fp32
roundings on the longest path of the kernel's reduction, is read off the kernel source and stated next to every function.

Terms that are new here
=======================
  * two-pass LayerNorm (two_pass): with n the additions on the longest path of ONE row reduction,
        mean:    e_m = gam(n + 1) sum |x| / D                         (+ 1: the division by D)
        centred: c = x - mean, e_c = e_m + u32 (|c| + e_m)            (one subtraction; the kernels recompute the same c in the affine step)
        squares: e_q = gam(n + 2) sum (|c| + e_c)^2 + sum (2 |c| e_c + e_c^2)      (+ 2: the square and the division by D)
        rstd:    the interval of q / D + eps is pushed through x^-1/2 by rsqrt_err (rsqrtf: 2^-22)
    No term carries the cancellation factor (sum x^2 / D + mean^2) / var of the one-pass form: on the `offset` rows (mean 200, deviation 1)
    that factor is 4e4 and a one-pass kernel loses three digits that this bound does not allow.  Where the input rows are themselves a
    kernel result (the second LayerNorm of assemble_preln) their error e_x enters every line above.
  * a wave dot product of length n: a lane adds ceil(n / 64) products one after the other, then the 6 xor steps of wave_sum:
    p = ceil(n / 64) + 6 + 1 (the product); a fused multiply-add only removes a rounding.
  * head_dense_kernel (fp32 MFMA): NO order is assumed -- gam(D + 1) sum |terms| holds for any order of D products and D additions.
  * sqrtf and `/`: the build passes neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt, so hipcc's default (correctly
    rounded fp32 division and square root) applies; the bound does not lean on that default and allows 1 ulp = 2^-23 for each (EPS_DIV).
  * __expf (small_mha): v_exp_f32 of x log2(e): 2^-22 for the instruction (as tests/attention_ref.py), u32 |x| each for the product and the
    rounded constant.  A factor common to all keys of a row (the rounding of the row maximum) cancels in e / sum(e).
Bit-exact comparisons carry no bound: pure copies, one fp32 operation followed by one correctly rounded bf16 conversion, zero padding.
The logits of the head are restated from the head's OWN returned codes (a separately bounded output), as normalize takes its statistics.
"""
import torch

from train_kernels_ref import (EPS_RSQ, LN_EPS, ROW_FAMILIES, TINY, U32, bf16_out, bits_equal, breaches, f32, gam, gen as _tr_gen, row_family,
                               rsqrt_err)

EPS_DIV = 2.0 ** -23                                   # one ulp of an fp32 division or square root
EPS_EXP = 2.0 ** -22                                   # v_exp_f32
F32 = torch.float32
BF16 = torch.bfloat16
LN_DEFECTS = ("one_pass", "eps_outside_sqrt", "sample_variance")


def gen(name, *key):
    return _tr_gen("forward/" + name, *key)


def cdiv(a, b):
    return -(-a // b)


def affine_params(D, tag):
    g = gen("affine", D, tag)
    return 1 + 0.3 * torch.randn(D, generator=g), 0.5 * torch.randn(D, generator=g)


# ---- two-pass LayerNorm -----------------------------------------------------------------------------------------------------------------
def two_pass(x, n, eps, e_x=None):
    """x [rows, D] fp64: the exact rows; e_x: what the fp32 rows the kernel holds may be off by (None: they are exact inputs); n: additions
    on the longest path of one row reduction.  Returns c = x - mean, rstd, e_c, e_r"""
    D = x.shape[1]
    e_x = torch.zeros_like(x) if e_x is None else e_x
    M = x.mean(1, keepdim=True)
    e_m = (gam(n + 1) * (x.abs() + e_x).sum(1, keepdim=True) + e_x.sum(1, keepdim=True)) / D
    c = x - M
    e_c = e_x + e_m + U32 * (c.abs() + e_x + e_m)
    A = (c * c).mean(1, keepdim=True)
    e_a = (gam(n + 2) * ((c.abs() + e_c) ** 2).sum(1, keepdim=True) + (2 * c.abs() * e_c + e_c ** 2).sum(1, keepdim=True)) / D
    W = A + eps
    R, e_r = rsqrt_err(W, e_a + U32 * (W + e_a))
    return c, R, e_c, e_r


def ln_affine(c, R, e_c, e_r, w, b):
    """y = ((c rstd) w) + b and the bound on the kernel's fp32 value: three roundings on top of the propagated errors"""
    xh = c * R
    e = c.abs() * e_r + e_c * (R + e_r)
    e = e + U32 * (xh.abs() + e)
    t = xh * w
    e = e * w.abs()
    e = e + U32 * (t.abs() + e)
    y = t + b
    return y, e + U32 * (y.abs() + e) + TINY


def ln_f32(x, w, b, eps, defect=None):
    """fp32 LayerNorm of fp32 rows with torch's reductions (another order than any kernel's)"""
    D = x.shape[1]
    e = torch.tensor(eps, dtype=F32)
    mean = x.sum(1, keepdim=True) / D
    c = x - mean
    if defect == "one_pass":
        var = ((x * x).sum(1, keepdim=True) / D - mean * mean).clamp_min(0)
    else:
        var = (c * c).sum(1, keepdim=True) / (D - 1 if defect == "sample_variance" else D)
    rstd = 1.0 / (var.sqrt() + e) if defect == "eps_outside_sqrt" else torch.rsqrt(var + e)
    return c * rstd * w + b


# layernorm_kernel / assemble_preln_kernel (row_stats): a lane adds x + y of each of its D / 128 pairs to its sum, then 6 butterfly steps:
# n = 1 + D / 128 + 6; the squares a a + b b take the place of x + y.
def n_row_stats(D):
    return 1 + D // 128 + 6


# layernorm_bf16_wide_kernel: a lane adds the 8 values of each of its ceil(D / 512) active 16-byte chunks one after the other, then 6 steps
def n_wide(D):
    return 8 * cdiv(D, 512) + 6


LN_D_F32 = (128, 384, 512, 1280)
LN_D_WIDE = (128, 384, 768, 1024)
LN_D_GENERIC = (128, 768, 1280)
LN_D_RULE = (1024, 1280)
LN_ROWS = (1, 5, 37)


def layernorm_ref(x, w, b, n, eps=LN_EPS):
    """x [rows, D] fp32 or bf16 (exact inputs) -> bf16((x - mean) rstd w + b): (y, bound)"""
    c, R, e_c, e_r = two_pass(x.double(), n, f32(eps))
    y, e_y = ln_affine(c, R, e_c, e_r, w.double(), b.double())
    return y, bf16_out(y, e_y)


def layernorm_emul(x, w, b, eps=LN_EPS, defect=None):
    return ln_f32(x.float(), w, b, eps, defect).to(BF16)


# ---- assemble_preln: rows from cls_pos0 / H / ctx, pre-LayerNorm -> H (fp32), LayerNorm of THAT -> xn (bf16) ------------------------------
ASSEMBLE_SHAPES = ((1, 6, 4, 128), (3, 9, 4, 384), (2, 23, 16, 1280))         # (B, ntok, np, D)
ASSEMBLE_DEFECTS = LN_DEFECTS + ("cls_from_H", "concept_off_by_one", "second_ln_of_source")


def assemble_inputs(B, ntok, np_, D, family):
    """H [B * ntok, D] (patch rows valid; row 0 and the concept rows NaN here -- the GPU test puts its sentinel there), cls_pos0, ctx,
    (pre_w, pre_b), (ln_w, ln_b)"""
    H = row_family(family, B * ntok, D, "assemble")
    t = torch.arange(B * ntok) % ntok
    H[(t == 0) | (t > np_)] = float("nan")
    Q = ntok - np_ - 1
    cls = row_family(family, 1, D, "assemble_cls")[0] * 0.5
    ctx = row_family(family, Q + 2, D, "assemble_ctx")[2:] * 1.5
    return H, cls, ctx, affine_params(D, "pre"), affine_params(D, "ln1")


def assemble_source_rows(H, ntok, np_, cls, ctx, defect=None):
    rows = H.shape[0]
    Q = ntok - np_ - 1
    t = torch.arange(rows) % ntok
    src = H.clone()
    if defect == "cls_from_H":
        src[t == 0] = H[(t == 1).nonzero()[0, 0]]
    else:
        src[t == 0] = cls
    qi = (t - np_ - 1)[t > np_]
    if defect == "concept_off_by_one":
        qi = (qi + 1) % Q
    src[t > np_] = ctx[qi]
    return src


def assemble_preln_ref(H, ntok, np_, cls, ctx, pre, ln, eps=LN_EPS):
    """(H_out, bound, xn, bound): the error of H_out is the input error of the second LayerNorm"""
    D = H.shape[1]
    n = n_row_stats(D)
    src = assemble_source_rows(H, ntok, np_, cls, ctx).double()
    c, R, e_c, e_r = two_pass(src, n, f32(eps))
    y1, e1 = ln_affine(c, R, e_c, e_r, pre[0].double(), pre[1].double())
    c, R, e_c, e_r = two_pass(y1, n, f32(eps), e1)
    y2, e2 = ln_affine(c, R, e_c, e_r, ln[0].double(), ln[1].double())
    return y1, e1, y2, bf16_out(y2, e2)


def assemble_preln_emul(H, ntok, np_, cls, ctx, pre, ln, eps=LN_EPS, defect=None):
    src = assemble_source_rows(H, ntok, np_, cls, ctx, defect)
    lnd = defect if defect in LN_DEFECTS else None
    y1 = ln_f32(src, pre[0], pre[1], eps, lnd)
    y2 = ln_f32(src if defect == "second_ln_of_source" else y1, ln[0], ln[1], eps, lnd)
    return y1, y2.to(BF16)


# ---- im2col: out[b Np + p][c patch^2 + ky patch + kx] = bf16(img[b][c][py patch + ky][px patch + kx]), zeros from K up to Kp: bit for bit ----
IM2COL_SHAPES = ((32, 16, 768), (28, 14, 640), (64, 32, 3072), (32, 8, 192), (32, 16, 832))         # (image, patch, Kp)
IM2COL_B = (1, 3)
IM2COL_DEFECTS = ("kx_ky_swapped", "padding_not_zero", "channel_stride_K")


def im2col_input(B, image, is_f32):
    x = torch.randn(B, 3, image, image, generator=gen("im2col", B, image))
    return x if is_f32 else x.to(BF16)


def im2col_ref(img, patch, Kp):
    B, _, image, _ = img.shape
    g = image // patch
    K = 3 * patch * patch
    cols = img.reshape(B, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, K).to(BF16)
    out = torch.zeros(B * g * g, Kp, dtype=BF16)
    out[:, :K] = cols
    return out


def im2col_emul(img, patch, Kp, defect=None):
    """the kernel's own index arithmetic, one output element at a time (vectorised over all of them)"""
    B, _, image, _ = img.shape
    g = image // patch
    pp = patch * patch
    K = 3 * pp
    idx = torch.arange(B * g * g * Kp)
    k, prow = idx % Kp, idx // Kp
    p, b = prow % (g * g), prow // (g * g)
    py, px = p // g, p % g
    kk = k.clamp_max(K - 1)
    c, rem = kk // pp, kk % pp
    ky, kx = rem // patch, rem % patch
    if defect == "kx_ky_swapped":
        ky, kx = kx, ky
    off = ((b * 3 + c) * image + py * patch + ky) * image + px * patch + kx
    if defect == "channel_stride_K":
        off = b * 3 * image * image + c * K + ((py * patch + ky) * image + px * patch + kx)
    v = img.reshape(-1)[off.clamp_max(img.numel() - 1)].to(BF16)
    if defect != "padding_not_zero":
        v = torch.where(k < K, v, torch.zeros_like(v))
    return v.view(B * g * g, Kp)


# ---- gather_head_rows: out[b (1 + ncon) + j] = H[b ntok + (j == 0 ? 0 : ntok - ncon + j - 1)]: bit for bit ----------------------------------
GATHER_SHAPES = ((1, 2, 1, 128), (5, 11, 4, 384))                                # (B, ntok, ncon, D)
GATHER_DEFECTS = ("concept_block_early", "cls_row_1")


def gather_head_rows_ref(H, B, ntok, ncon):
    v = H.view(B, ntok, -1)
    return torch.cat([v[:, :1], v[:, ntok - ncon:]], 1).reshape(B * (1 + ncon), -1).contiguous()


def gather_head_rows_emul(H, B, ntok, ncon, defect=None):
    out = torch.zeros(B * (1 + ncon), H.shape[-1], dtype=H.dtype)
    c0 = ntok - ncon - (1 if defect == "concept_block_early" else 0)
    for r in range(B * (1 + ncon)):
        b, j = divmod(r, 1 + ncon)
        out[r] = H[b * ntok + ((1 if defect == "cls_row_1" else 0) if j == 0 else c0 + j - 1)]
    return out


# ---- the hashing head -----------------------------------------------------------------------------------------------------------------------
# (D, Q, nbit, B, C, P, ntok): row tiles of the dense kernel 4 | 5 | 20 | 68 rows (B Q) and 1 | 5 | 17 rows (B), column tiles of 1 | 37 | 200 and
# 16 | 40 columns, one or several 64-bit words of packed codes, ntok = Q + 1 (the CLS row right in front of the concept rows) and 11
HEAD_SHAPES = ((128, 4, 16, 1, 1, 16, 5), (128, 1, 16, 5, 37, 40, 2), (384, 4, 48, 5, 200, 40, 11), (384, 4, 128, 17, 37, 16, 11),
               (128, 1, 48, 17, 200, 16, 11), (384, 1, 128, 1, 37, 40, 11))
HEAD_OUTPUTS = ("packed", "logits_cont", "logits_bin", "logits_concept", "hash_features", "image_features")
HEAD_DEFECTS = ("concept_bc_layout", "row_clamp_off_by_one", "pack_ge", "no_normalize_eps", "cls_one_pass", "cls_eps_outside_sqrt",
                "cls_sample_variance", "codes_without_pe", "bin_from_cont_centres")
HEAD_CLS_FAMILIES = ("offset", "scaled", "benign", "outlier", "constant")
HEAD_REFUSALS = (dict(D=128, Q=4, nbit=18), dict(D=100, Q=4, nbit=16), dict(D=384, Q=64, nbit=64))     # nbit % Q, D % 16, Q D past the LDS


def head_inputs(D, Q, nbit, B, C, P, ntok):
    """The CLS row of image b is a row of family HEAD_CLS_FAMILIES[b % 5].  Special rows (only where B >= 5, so that the small cases stay plain): image 1's concept row 0 is exactly -concept_pe[0] (its l2 norm
    is zero: the F.normalize eps path); bits 3 and 5 have bn_scale = 0 with bn_shift = +0 / -0 (a code of exactly +0, and of -0 wherever the
    dot product is negative); image 2 has ALL its codes zero in a second set of BN constants (bn_scale = bn_shift = 0), see head_zero_bn."""
    g = gen("head", D, Q, nbit, B, C, P, ntok)
    r = lambda *s: torch.randn(*s, generator=g)
    sub = nbit // Q
    i = dict(H=r(B * ntok, D), hash_pe=0.3 * r(Q, D), hash_fc=r(sub, D) * D ** -0.5, bn_scale=1 + 0.3 * r(nbit), bn_shift=0.2 * r(nbit),
             concept_pe=0.3 * r(Q, D), post_w=1 + 0.3 * r(D), post_b=0.5 * r(D), vis_proj=r(P, D) * D ** -0.5)
    cl = r(C, nbit)
    cl = cl / cl.norm(dim=1, keepdim=True)
    i["center_l2"] = cl
    i["center_bin"] = torch.sign(cl) * nbit ** -0.5
    cc = r(C, D)
    i["concept_cent_l2"] = cc / cc.norm(dim=1, keepdim=True)
    for b in range(B):                                    # the CLS rows go through a LayerNorm: every row family, the offset rows first
        i["H"].view(B, ntok, D)[b, 0] = row_family(HEAD_CLS_FAMILIES[b % 5], 1, D, f"head_cls/{b}")[0]
    if B >= 5:
        i["H"].view(B, ntok, D)[1, ntok - Q] = -i["concept_pe"][0]
        i["bn_scale"][3], i["bn_shift"][3] = 0.0, 0.0
        i["bn_scale"][5], i["bn_shift"][5] = 0.0, -0.0
    return i


def head_zero_bn(i):
    """the same inputs with bn_scale = bn_shift = 0 on every bit: every code of every image is +0 or -0"""
    j = dict(i)
    j["bn_scale"], j["bn_shift"] = torch.zeros_like(i["bn_scale"]), torch.zeros_like(i["bn_shift"])
    return j


def _hash_rows(H, B, ntok, Q):
    return H.view(B, ntok, -1)[:, ntok - Q:]


def head_codes_ref(i, B, ntok, Q, nbit):
    """codes [B, nbit] = (sum_k (x_c + pe_c)[k] w_s[k]) scale + shift, o = c sub + s.  A wave dot of length D on the sums x + pe (one more
    rounding): p = ceil(D / 64) + 6 + 2; then the product with the scale and the addition of the shift.  Also returns the exact dot products."""
    D = i["H"].shape[1]
    x = _hash_rows(i["H"], B, ntok, Q).double() + i["hash_pe"].double()                       # [B, Q, D]
    w = i["hash_fc"].double()
    acc = torch.einsum("bqd,sd->bqs", x, w).reshape(B, nbit)
    e_acc = gam(cdiv(D, 64) + 8) * torch.einsum("bqd,sd->bqs", x.abs(), w.abs()).reshape(B, nbit)
    sc, sh = i["bn_scale"].double(), i["bn_shift"].double()
    t = acc * sc
    e = e_acc * sc.abs()
    e = e + U32 * (t.abs() + e)
    v = t + sh
    return v, e + U32 * (v.abs() + e) + TINY, acc, e_acc


def inv_norm(s, e_s):
    """1 / max(sqrt(s), 1e-12f) for |s' - s| <= e_s, s >= 0: (inv, e_inv); sqrtf and the division 1 ulp each"""
    n = s.sqrt()
    e_n = torch.maximum((s + e_s).sqrt() - n, n - (s - e_s).clamp_min(0).sqrt())
    e_n = e_n + EPS_DIV * (n + e_n)
    floor = f32(1e-12)
    m = n.clamp_min(floor)                                                                     # max(., c) is 1-Lipschitz
    lo = (m - e_n).clamp_min(floor)
    inv = 1.0 / m
    return inv, (1.0 / lo - inv) + EPS_DIV / lo


def head_logits_ref(codes, centres):
    """logits [B, C] = (sum_i codes[i] centres[c][i]) / max(|codes|, 1e-12) from the head's own fp32 codes (exact inputs here).  A thread adds
    the nbit products in order: p = nbit + 1; |codes|^2 is a wave dot: p = ceil(nbit / 64) + 7."""
    nbit = codes.shape[1]
    cd, ce = codes.double(), centres.double()
    a = cd @ ce.t()
    e_a = gam(nbit + 1) * (cd.abs() @ ce.abs().t())
    s = (cd * cd).sum(1, keepdim=True)
    inv, e_inv = inv_norm(s, gam(cdiv(nbit, 64) + 7) * s)
    v = a * inv
    e = e_a * (inv + e_inv) + a.abs() * e_inv
    return v, e + U32 * (v.abs() + e) + TINY


def _dense(X, e_X, W):
    """out = X W^T by the fp32 MFMA, any order: D products and D additions"""
    D = X.shape[-1]
    Wd = W.double()
    out = X @ Wd.t()
    dense = gam(D + 1) * ((X.abs() + e_X) @ Wd.abs().t())
    return out, e_X @ Wd.abs().t() + dense + TINY, dense + TINY


def head_concept_ref(i, B, ntok, Q):
    """logits_concept [Q, B, C]: v = x_c + concept_pe_c (one rounding); |v|^2 over 256 threads: ceil(D / 256) additions, 6 butterfly steps, 3 to
    add the four waves, the square: p = ceil(D / 256) + 10; xn = v inv; then the dense product with the l2-normalised centroids.
    Returns (ref, bound, the dense product's own share of the bound)"""
    D = i["H"].shape[1]
    v = _hash_rows(i["H"], B, ntok, Q).double() + i["concept_pe"].double()
    e_v = U32 * v.abs()
    s = (v * v).sum(-1, keepdim=True)
    e_s = gam(cdiv(D, 256) + 10) * ((v.abs() + e_v) ** 2).sum(-1, keepdim=True) + (2 * v.abs() * e_v + e_v ** 2).sum(-1, keepdim=True)
    inv, e_inv = inv_norm(s, e_s)
    xn = v * inv
    e = e_v * (inv + e_inv) + v.abs() * e_inv
    e = e + U32 * (xn.abs() + e)
    out, bound, dense = _dense(xn, e, i["concept_cent_l2"])                                       # [B, Q, C]
    return out.permute(1, 0, 2).contiguous(), bound.permute(1, 0, 2).contiguous(), dense.permute(1, 0, 2).contiguous()


def n_head_cls(D):
    """the CLS LayerNorm of head_kernel: ceil(D / 256) additions per thread, 6 butterfly steps, 3 to add the four waves"""
    return cdiv(D, 256) + 9


def head_image_features_ref(i, B, ntok):
    """image_features [B, P] = vis_proj (post_layernorm(H[b, 0])): the two-pass LayerNorm, then the dense product"""
    D = i["H"].shape[1]
    h0 = i["H"].view(B, ntok, D)[:, 0].double()
    c, R, e_c, e_r = two_pass(h0, n_head_cls(D), f32(LN_EPS))
    y, e_y = ln_affine(c, R, e_c, e_r, i["post_w"].double(), i["post_b"].double())
    return _dense(y, e_y, i["vis_proj"])


def pack_codes(codes, ge=False):
    """[B, ceil(nbit / 64)] int64 words, bit i of word w = codes[64 w + i] > 0"""
    B, nbit = codes.shape
    W = cdiv(nbit, 64)
    bits = torch.zeros(B, W * 64, dtype=torch.int64)
    bits[:, :nbit] = ((codes >= 0) if ge else (codes > 0)).to(torch.int64)
    sh = torch.arange(64, dtype=torch.int64)
    # bit 63 set makes the word negative in two's complement: shifting in int64 wraps to exactly that pattern
    return (bits.view(B, W, 64) << sh).sum(-1)


def head_emul(i, B, ntok, Q, nbit, defect=None):
    """every output of the head in fp32 with torch's reductions; the logits from its own codes"""
    D = i["H"].shape[1]
    hf = _hash_rows(i["H"], B, ntok, Q).contiguous()
    x = hf if defect == "codes_without_pe" else hf + i["hash_pe"]
    codes = (x @ i["hash_fc"].t()).reshape(B, nbit) * i["bn_scale"] + i["bn_shift"]
    nrm = codes.norm(dim=1, keepdim=True)
    inv = 1.0 / (nrm if defect == "no_normalize_eps" else nrm.clamp_min(1e-12))
    cont = (codes @ i["center_l2"].t()) * inv
    cbin = (codes @ (i["center_l2"] if defect == "bin_from_cont_centres" else i["center_bin"]).t()) * inv
    v = hf + i["concept_pe"]
    nv = v.norm(dim=-1, keepdim=True)
    xn = (v / (nv if defect == "no_normalize_eps" else nv.clamp_min(1e-12))).reshape(B * Q, D)
    if defect == "row_clamp_off_by_one":
        xn = xn[torch.arange(B * Q).clamp_max(B * Q - 2 if B * Q > 1 else 0)]
    con = (xn @ i["concept_cent_l2"].t()).view(B, Q, -1)
    C = con.shape[-1]
    con = con.reshape(Q, B, C) if defect == "concept_bc_layout" else con.permute(1, 0, 2).contiguous()
    lnd = defect[4:] if defect in ("cls_one_pass", "cls_eps_outside_sqrt", "cls_sample_variance") else None
    cls = ln_f32(i["H"].view(B, ntok, D)[:, 0], i["post_w"], i["post_b"], LN_EPS, lnd)
    return dict(codes=codes, packed=pack_codes(codes, ge=defect == "pack_ge"), logits_cont=cont, logits_bin=cbin, logits_concept=con,
                hash_features=hf, image_features=cls @ i["vis_proj"].t())


def head_wrong(res, i, B, ntok, Q, nbit):
    """True when a result set (dict as head_emul's; all outputs) leaves a bound or a bit-exact comparison"""
    codes, e_codes, _, _ = head_codes_ref(i, B, ntok, Q, nbit)
    bad = breaches(res["codes"], codes, e_codes)
    bad |= not torch.equal(res["packed"], pack_codes(res["codes"]))
    bad |= not bits_equal(res["hash_features"], _hash_rows(i["H"], B, ntok, Q).contiguous())
    if not bool(torch.isfinite(res["codes"]).all()):
        return True
    bad |= breaches(res["logits_cont"], *head_logits_ref(res["codes"], i["center_l2"]))
    bad |= breaches(res["logits_bin"], *head_logits_ref(res["codes"], i["center_bin"]))
    bad |= breaches(res["logits_concept"], *head_concept_ref(i, B, ntok, Q)[:2])
    bad |= breaches(res["image_features"], *head_image_features_ref(i, B, ntok)[:2])
    return bad


# ---- small_linear: y = act(x W^T + b): a wave dot of length in_f, the bias: p = ceil(in_f / 64) + 8; relu is exact and 1-Lipschitz ----------
LINEAR_SHAPES = ((1, 1, 1), (4, 100, 7), (3, 512, 130))                          # (rows, in_f, out_f)
LINEAR_DEFECTS = ("no_bias", "no_act", "bias_of_row")


def linear_inputs(rows, in_f, out_f):
    g = gen("small_linear", rows, in_f, out_f)
    return torch.randn(rows, in_f, generator=g), torch.randn(out_f, in_f, generator=g) * in_f ** -0.5, torch.randn(out_f, generator=g)


def small_linear_ref(x, W, b, act):
    xd, Wd = x.double(), W.double()
    y = xd @ Wd.t()
    mag = xd.abs() @ Wd.abs().t()
    if b is not None:
        y, mag = y + b.double(), mag + b.double().abs()
    return (y.clamp_min(0) if act == 1 else y), gam(cdiv(x.shape[1], 64) + 8) * mag + TINY


def small_linear_emul(x, W, b, act, defect=None):
    y = x.flip(1) @ W.flip(1).t()
    if b is not None and defect != "no_bias":
        y = y + (b[torch.arange(y.shape[0]) % b.numel()][:, None] if defect == "bias_of_row" else b)
    return y.clamp_min(0) if act == 1 and defect != "no_act" else y


# ---- small_layernorm: fp32 rows -> fp32, any D: a lane adds ceil(D / 64) values, 6 butterfly steps ------------------------------------------
SMALL_LN_D = (1, 100, 512)
SMALL_LN_ROWS = (1, 5)
SMALL_LN_FAMILIES = ("benign", "scaled", "offset")


def n_small_ln(D):
    return cdiv(D, 64) + 6


def small_layernorm_ref(x, w, b, eps=LN_EPS):
    c, R, e_c, e_r = two_pass(x.double(), n_small_ln(x.shape[1]), f32(eps))
    return ln_affine(c, R, e_c, e_r, w.double(), b.double())


# ---- small_add: one fp32 addition: bit for bit -------------------------------------------------------------------------------------------------
ADD_N = (1, 257)


# ---- small_mha: softmax(q k^T / sqrt(hd)) v per (head, query), T <= 64 keys, one per lane ------------------------------------------------------
MHA_SHAPES = ((1, 64, 8), (4, 512, 8), (64, 128, 4), (33, 96, 3))               # (T, P, heads)
MHA_DEFECTS = ("scale_1_over_hd", "last_key_dropped", "heads_interleaved", "values_from_keys")


def mha_input(T, P, heads):
    """qkv [T, 3 P]; scores of deviation ~ 2 (a peaked but not one-hot softmax)"""
    x = torch.randn(T, 3 * P, generator=gen("small_mha", T, P, heads))
    x[:, :2 * P] *= 2.0 ** 0.5                               # q . k / sqrt(hd) has deviation 2
    return x


def _mha_split(qkv, T, P, heads):
    hd = P // heads
    q, k, v = (qkv[:, j * P:(j + 1) * P].reshape(T, heads, hd).permute(1, 0, 2) for j in range(3))
    return q, k, v, hd


def small_mha_ref(qkv, T, P, heads):
    """the score: hd products added in order: gam(hd + 1); times rsqrtf(hd) (2^-22) with one product; t = sc - max (u32 |t|, and the
    maximum's own error is common to the row); __expf: (2 u32 |t| + 2^-22); the denominator: 6 butterfly steps; e / sum: 1 ulp; the output:
    one product and 6 butterfly steps"""
    q, k, v, hd = (t.double() if torch.is_tensor(t) else t for t in _mha_split(qkv, T, P, heads))
    sc = hd ** -0.5
    s = q @ k.transpose(1, 2) * sc                                                                # [heads, T, T]
    e_s = gam(hd + 1) * (q.abs() @ k.abs().transpose(1, 2)) * sc
    e_s = e_s + ((1 + EPS_RSQ) * (1 + U32) - 1) * (s.abs() + e_s)
    t = s - s.max(-1, keepdim=True).values
    ta = t.abs() + 2 * e_s.max(-1, keepdim=True).values
    eps_j = torch.expm1(e_s + 3 * U32 * ta + EPS_EXP)
    p = torch.softmax(s, -1)
    beta = (p * ((1 + eps_j) * (1 + gam(6)) - 1)).sum(-1, keepdim=True)
    alpha = (1 + eps_j) * (1 + EPS_DIV) * (1 + gam(7)) / (1 - beta) - 1
    o = p @ v
    # out - o = sum_j p_j v_j ((1 + theta_j)(1 + division)(1 + product, butterfly) / (1 + b) - 1), |b| <= beta: every factor is inside alpha_j
    bound = (p * alpha) @ v.abs() + TINY * (1 + v.abs().max())
    return o.permute(1, 0, 2).reshape(T, P), bound.permute(1, 0, 2).reshape(T, P)


def small_mha_emul(qkv, T, P, heads, defect=None):
    if defect == "heads_interleaved":                       # head h at columns h, h + heads, ... instead of h hd .. h hd + hd - 1
        hd = P // heads
        q, k, v = (qkv[:, j * P:(j + 1) * P].reshape(T, hd, heads).permute(2, 0, 1) for j in range(3))
    else:
        q, k, v, hd = _mha_split(qkv, T, P, heads)
    s = q @ k.transpose(1, 2) * (1.0 / hd if defect == "scale_1_over_hd" else hd ** -0.5)
    if defect == "values_from_keys":                        # the only defect that one key (T = 1: the output is v itself) can show
        v = k
    if defect == "last_key_dropped" and T > 1:
        s = s[..., :-1]
        v = v[:, :-1]
    o = torch.softmax(s, -1) @ v
    if defect == "heads_interleaved":
        return o.permute(1, 2, 0).reshape(T, P)
    return o.permute(1, 0, 2).reshape(T, P)


# ---- small_l2norm: out_l2 = x / max(|x|, 1e-12); out_bin = sign(out_l2) rsqrtf(cols) -----------------------------------------------------------
L2_SHAPES = ((1, 16), (5, 100), (37, 384))
L2_DEFECTS = ("no_normalize_eps", "bin_of_input_ge", "norm_of_neighbour")


def l2_input(rows, cols):
    """row 0 is the zero row where there is more than one row, and the only row of the 1 x 16 case keeps one exact zero element"""
    x = torch.randn(rows, cols, generator=gen("l2norm", rows, cols)) * torch.exp2(torch.arange(rows) % 9 - 4.0)[:, None]
    if rows > 1:
        x[0] = 0
    x[-1, 3] = 0
    return x


def small_l2norm_ref(x):
    """|x|^2: a wave dot: p = ceil(cols / 64) + 7; sqrtf, the division, the product.  Returns (l2, bound, |bin| = cols^-1/2, its bound)"""
    xd = x.double()
    s = (xd * xd).sum(1, keepdim=True)
    inv, e_inv = inv_norm(s, gam(cdiv(x.shape[1], 64) + 7) * s)
    v = xd * inv
    e = xd.abs() * e_inv
    bs = x.shape[1] ** -0.5
    return v, e + U32 * (v.abs() + e) + TINY, bs, EPS_RSQ * bs


def small_l2norm_emul(x, defect=None):
    n = x.norm(dim=1, keepdim=True)
    if defect == "norm_of_neighbour":
        n = n.roll(1, 0) if x.shape[0] > 1 else n * 2
    l2 = x / (n if defect == "no_normalize_eps" else n.clamp_min(1e-12))
    bs = torch.rsqrt(torch.tensor(float(x.shape[1])))
    if defect == "bin_of_input_ge":
        return l2, torch.where(x >= 0, bs, -bs)
    return l2, torch.sign(l2) * bs


def l2_wrong(l2, bn, x):
    ref, bound, bs, e_bs = small_l2norm_ref(x)
    if breaches(l2, ref, bound):
        return True
    return not torch.equal(torch.sign(bn), torch.sign(l2)) or bool(((bn.double().abs() - bs).abs()[bn != 0] > e_bs).any())


# ---- convert_bf16: [rows, cols] fp32 -> [rows, cols_pad] bf16, zero padded: bit for bit ---------------------------------------------------------
CONVERT_SHAPES = ((1, 8, 8), (3, 588, 640), (5, 100, 104))


def convert_bf16_ref(x, cols_pad):
    out = torch.zeros(x.shape[0], cols_pad, dtype=BF16)
    out[:, :x.shape[1]] = x.to(BF16)
    return out


# ---- bn_fold: scale = w / sqrt(var + eps), shift = b - mean scale -----------------------------------------------------------------------------
BN_N = (16, 300)
BN_EPS = 1e-5
BN_DEFECTS = ("shift_unscaled_mean", "eps_outside_sqrt", "shift_plus")


def bn_inputs(n):
    """(w, b, mean, var); var = 0 at elements 0 and 7"""
    g = gen("bn_fold", n)
    w, b, mean = 1 + 0.3 * torch.randn(n, generator=g), 0.2 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    var = torch.rand(n, generator=g) * 2 + 0.05
    var[0] = var[7] = 0.0
    return w, b, mean, var


def bn_fold_ref(w, b, mean, var, eps=BN_EPS):
    """var + eps (u32), sqrtf (1 ulp on half the relative error before it), the division (1 ulp); shift: one product, one subtraction"""
    wd, bd, md, vd = (t.double() for t in (w, b, mean, var))
    sc = wd / (vd + f32(eps)).sqrt()
    e_sc = sc.abs() * ((1 + U32) * (1 + EPS_DIV) ** 2 - 1)
    t = md * sc
    e = md.abs() * e_sc
    e = e + U32 * (t.abs() + e)
    sh = bd - t
    return sc, e_sc + TINY, sh, e + U32 * (sh.abs() + e) + TINY


def bn_fold_emul(w, b, mean, var, eps=BN_EPS, defect=None):
    e = torch.tensor(eps, dtype=F32)
    sc = w / (var.sqrt() + e) if defect == "eps_outside_sqrt" else w * torch.rsqrt(var + e)
    if defect == "shift_unscaled_mean":
        return sc, b - mean
    return sc, (b + mean * sc) if defect == "shift_plus" else (b - mean * sc)


# ---- fold_ln: Wdf = bf16(Wd gamma) (rows past b zero), c[n] = sum_k float(Wdf[n][k]), d[n] = sum_k beta[k] Wd[n][k] + bd[n] --------------------
FOLD_LN_SHAPES = ((5, 128, 128), (130, 256, 384), (384, 384, 768))              # (b, bpad, D)
FOLD_LN_DEFECTS = ("c_unrounded", "d_without_bias", "padding_not_zero", "d_of_folded_weight")


def fold_ln_inputs(b, D):
    g = gen("fold_ln", b, D)
    return (torch.randn(b, D, generator=g) * D ** -0.5, 0.1 * torch.randn(b, generator=g), 1 + 0.3 * torch.randn(D, generator=g),
            0.5 * torch.randn(D, generator=g))


def fold_ln_ref(Wd, bd, gamma, beta, bpad):
    """(Wdf exact bf16 [bpad, D], c, bound, d, bound): wave dots of length D: p = ceil(D / 64) + 6 for c (no product: the addends are the
    rounded weights), + 2 for d (the product, the bias)"""
    b, D = Wd.shape
    wdf = torch.zeros(bpad, D, dtype=BF16)
    wdf[:b] = (Wd * gamma[None, :]).to(BF16)
    p = cdiv(D, 64) + 6
    c = wdf.double().sum(1)
    d = torch.zeros(bpad, dtype=torch.float64)
    terms = Wd.double() * beta.double()[None, :]
    d[:b] = terms.sum(1) + bd.double()
    e_d = torch.full((bpad,), TINY, dtype=torch.float64)
    e_d[:b] += gam(p + 2) * (terms.abs().sum(1) + bd.double().abs())
    return wdf, c, gam(p) * wdf.double().abs().sum(1) + TINY, d, e_d


def fold_ln_emul(Wd, bd, gamma, beta, bpad, defect=None):
    b, D = Wd.shape
    prod = Wd * gamma[None, :]
    wdf = torch.zeros(bpad, D, dtype=BF16)
    wdf[:b] = prod.to(BF16)
    c, d = torch.zeros(bpad), torch.zeros(bpad)
    c[:b] = (prod if defect == "c_unrounded" else wdf[:b].float()).flip(1).sum(1)
    d[:b] = ((prod if defect == "d_of_folded_weight" else Wd) * beta[None, :]).flip(1).sum(1) + (0 if defect == "d_without_bias" else bd)
    if defect == "padding_not_zero" and bpad > b:
        wdf[b], c[b], d[b] = wdf[b - 1], c[b - 1], d[b - 1]
    return wdf, c, d


def fold_ln_wrong(res, Wd, bd, gamma, beta, bpad):
    b = Wd.shape[0]
    wdf, c, e_c, d, e_d = fold_ln_ref(Wd, bd, gamma, beta, bpad)
    bad = not bits_equal(res[0][:b].contiguous(), wdf[:b].contiguous()) or bool(res[0][b:].float().any())
    bad |= breaches(res[1], c, e_c) or breaches(res[2], d, e_d)
    return bad or bool(res[1][b:].any()) or bool(res[2][b:].any())
