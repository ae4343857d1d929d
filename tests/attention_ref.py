"""Plain fp64 reference for the forward attention kernels, softmax(q k^T / 8) v on bf16-rounded inputs (head_dim 64), with a DERIVED
elementwise error bound, seeded input builders, and a torch emulation of the kernels' arithmetic (CPU test + GPU tests share all of it).

Layout: qkv [B * ntok, 3 * heads * 64] bf16 (q | k | v, head h at columns h * 64), out [B * ntok, heads * 64], as the kernels.

The bound
=========
u = 2^-8 (bf16 unit roundoff, round to nearest even: ch_common.h pack_bf16x2), u32 = 2^-24, gamma_n = n u32 / (1 - n u32) (the standard
bound on n fp32 roundings in any order), c = log2(e) / 8.  For one query, exact scores s_j = q . k_j, exact probabilities p_j, exact
output o_d = sum_j p_j v_jd, and A_d = sum_j p_j |v_jd|.  The kernel's UNNORMALISED weight of key j is, up to a factor common to all
keys of the row (which cancels in the quotient, so the rounding of `mxs` does not matter), w_j = p_j (1 + theta_j) with
|theta_j| <= eps_j = expm1(x_j):

  x_j =  gamma_64 S_j / 8                      S_j = sum_d |q_d| |k_jd|: the score is two chained v_mfma_f32_16x16x32_bf16, 64 products
                                               accumulated in fp32 (attention.hip:124-125, attention_stream.hip:127-128); d(ln w)/ds = 1/8
       + ln2 u32 (c |s_j| + 2 |t_j|)           t_j = (s_j - max_i s_i) c: the product `st * scale_log2e` (u32 c |s_j|), the fp32 constant
                                               scale_log2e itself (u32 |t_j|) and the subtraction (u32 |t_j|) (attention.hip:170,
                                               attention_stream.hip:154); fused or not, the same bound holds
       + 2^-22                                 v_exp_f32 (1 ulp, __builtin_amdgcn_exp2f, same lines)

  streaming kernel, per-block rescale (attention_stream.hip:146-160): the weights of a block are multiplied, in the numerator AND in
  the denominator by the same fp32 numbers, by alpha of every later block, alpha = exp2((m - mn) c):
       + ln2 3 u32 |t_j|                       the subtraction, the product and the constant inside the alphas; their exponents sum to
                                               (block maximum - final maximum) c, at most |t_j| in magnitude
       + (NB - 1) 2^-22                        one v_exp_f32 per later block, NB = ceil(ntok / 64) blocks
  and `l * alpha + bs`, `o *= alpha` add 2 NB + 2 fp32 roundings to the two accumulations below.

The numerator rounds w_j to bf16 as the B operand of the P V product (attention.hip:220-223, attention_stream.hip:171-174) and
accumulates KP products in fp32 MFMAs (attention.hip:225, attention_stream.hip:176; KP = keys padded to 32 / 64, the padded ones have
weight exactly 0); the denominator is the fp32 sum of the UNROUNDED weights (attention.hip:172-175, attention_stream.hip:156-158, 180-181):

  numerator   N_d = sum_j p_j v_jd (1 + a_j),  |a_j| <= alpha_j = (1 + eps_j)(1 + u)(1 + gamma_n) - 1        n = KP (+ 2 NB + 2 streaming)
  denominator D   = 1 + b,                     |b|   <= beta    = sum_j p_j ((1 + eps_j)(1 + gamma_n) - 1)
  |N_d / D - o_d| <= (E_d + |o_d| beta) / (1 - beta),   E_d = sum_j p_j alpha_j |v_jd|

then `inv = 1.0f / sum` (at most 1 ulp, 2^-23, for the IEEE division or v_rcp_f32) and `o * inv` (u32), tau = (1 + 2^-23)(1 + u32) - 1,
and the bf16 rounding of the output (attention.hip:233-234, attention_stream.hip:214-215):

  E1_d  = (E_d + |o_d| beta) / (1 - beta) (1 + tau) + |o_d| tau
  bound = E1_d (1 + u) + u |o_d| + 2^-100 max|v|

To first order this is u (A_d + |o_d|) plus the fp32 terms.  The last term covers weights that v_exp_f32 flushes to zero (results
below 2^-126, relative to a largest weight of 1) and fp32 / bf16 subnormals.

Tapped probabilities (attention.hip:187, attention_stream.hip:203) are w_j * inv in fp32, no bf16 rounding:
  |tap_j - p_j| <= p_j ((1 + eps_j)(1 + tau) / (1 - beta) - 1) + 2^-100
The streaming kernel's second pass recomputes the score with the same two MFMAs and uses the final (m, l): the same bound.

Second-order products of these terms are covered by gamma_n >= n u32 and by taking 2^-22 for the documented 1 ulp (2^-23) of v_exp_f32.
"""
import math
import zlib

import torch

HD = 64
U = 2.0 ** -8
U32 = 2.0 ** -24
EPS_EXP2 = 2.0 ** -22
EPS_RCP = 2.0 ** -23
C = math.log2(math.e) / 8.0
TINY = 2.0 ** -100
BK = 64                                   # key block of the streaming kernel
BUILDERS = ("benign", "peaked", "offset", "last_key")
STREAM_BUILDERS = BUILDERS + ("ascending", "descending")
DEFECTS = ("drop_last", "dup_last", "causal_plus", "causal_minus", "tap_shift")
# the cases of tests/test_attention_fwd_gpu.py; tests/test_attention_ref_cpu.py walks the same ones
B_TEST, H_TEST = 3, 3
RESIDENT_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 287, 288)
CAUSAL_LENGTHS = (1, 2, 16, 17, 32, 33, 77, 128, 129, 257, 288)
CAUSAL_BUILDERS = ("benign", "peaked", "offset")
STREAM_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 320, 1024, 1088)         # with 4 concept tokens; and
STREAM_MAX = (1089, 64)                                                   # the documented maximum: 1089 tokens, 64 of them concept tokens
STREAM_NCON = 4
TAP_NCON = (1, 4, 15, 16, 17, 64)
TAP_BUILDERS = ("benign", "peaked")


def tap_lengths(ncon):
    return tuple(sorted({ncon + 2, 201, 288}))


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def split(qkv, B, n, H):
    """[B*n, 3*H*64] -> q, k, v as [B, H, n, 64] fp64 (only the first B*n rows are looked at)"""
    t = qkv[:B * n].double().view(B, n, 3, H, HD).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def merge(o):
    """[B, H, n, 64] -> [B*n, H*64]"""
    B, H, n, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(B * n, H * HD)


def causal_mask(n, device, shift=0):
    """True where key > query + shift (masked)"""
    i = torch.arange(n, device=device)
    return i[None, :] > i[:, None] + shift


def reference(qkv, B, n, H, causal=False):
    """fp64 attention: (out [B*n, H*64], p [B, H, n, n])"""
    q, k, v = split(qkv, B, n, H)
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(causal_mask(n, s.device), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return merge(p @ v), p


def tapped(p, ncon, shift=0):
    """the rows the kernels' tap writes: p[:, :, -ncon:, 1:-ncon]"""
    n = p.shape[-1]
    return p[:, :, n - ncon:, 1 - shift:n - ncon - shift]


def head_rows(B, n, ncon):
    """rows of the full output that compact mode keeps: CLS and the last ncon tokens of every image"""
    return torch.tensor([b * n + t for b in range(B) for t in [0] + list(range(n - ncon, n))])


def bounds(qkv, B, n, H, causal=False, streaming=False):
    """(out, out_bound [B*n, H*64], p, p_bound [B, H, n, n]), all fp64: the derivation of the module docstring, term by term"""
    q, k, v = split(qkv, B, n, H)
    s = q @ k.transpose(-1, -2)                                    # raw scores
    S = q.abs() @ k.abs().transpose(-1, -2)
    if causal:
        mask = causal_mask(n, s.device)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s / 8.0, dim=-1)
    t = (s - s.max(-1, keepdim=True).values) * C
    if causal:
        t = t.masked_fill(mask, 0.0)                               # p = 0 there: the term carries no weight
        s = s.masked_fill(mask, 0.0)
    blk = BK if streaming else 32
    KP = (n + blk - 1) // blk * blk
    NB = KP // BK
    x = gamma(64) * S / 8.0 + math.log(2.0) * U32 * (C * s.abs() + 2.0 * t.abs()) + EPS_EXP2
    nacc = KP
    if streaming:
        x = x + math.log(2.0) * 3.0 * U32 * t.abs() + (NB - 1) * EPS_EXP2
        nacc = KP + 2 * NB + 2
    eps = torch.expm1(x)
    g = gamma(nacc)
    alpha = (1.0 + eps) * (1.0 + U) * (1.0 + g) - 1.0
    beta = (p * ((1.0 + eps) * (1.0 + g) - 1.0)).sum(-1, keepdim=True)
    o = p @ v
    E = (p * alpha) @ v.abs()
    tau = (1.0 + EPS_RCP) * (1.0 + U32) - 1.0
    E1 = (E + o.abs() * beta) / (1.0 - beta) * (1.0 + tau) + o.abs() * tau
    out_bound = E1 * (1.0 + U) + U * o.abs() + TINY * float(v.abs().max())
    p_bound = p * ((1.0 + eps) * (1.0 + tau) / (1.0 - beta) - 1.0) + TINY
    return merge(o), merge(out_bound), p, p_bound


def assert_within(got, ref, bound, what):
    """THE assertion of the GPU tests and of the CPU test: every element finite and within its bound.  Prints and returns the worst
    error / bound ratio."""
    got = got.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    ratio = float(((got - ref).abs() / bound).max()) if got.numel() else 0.0
    print(f"{what}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error exceeds the derived bound, worst ratio {ratio:.3f}"
    return ratio


# ---- seeded inputs: CPU generator, the same bytes on every machine -----------------------------------------------------------------
def _gen(name, n, seed):
    return torch.Generator().manual_seed(zlib.crc32(f"{name}/{n}/{seed}".encode()))


def _unit(g, B, H):
    d = torch.randn(B, 1, H, HD, generator=g)
    return d / d.norm(dim=-1, keepdim=True)


def build(name, B, n, H, seed=0):
    """qkv [B*n, 3*H*64] bf16 on the CPU"""
    g = _gen(name, n, seed)
    x = 1.5 * torch.randn(B, n, 3, H, HD, generator=g)            # benign: the distribution of the existing tests
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]                  # views, [B, n, H, 64]
    if name == "benign":
        pass
    elif name == "peaked":
        # scaled logits with a standard deviation of 4^2 = 16 (what keeps the median row maximum above 0.9 up to 1089 keys): near one-hot rows; an eighth of the keys are near copies of another key
        # (groups of two and of three), so a row whose top key is one of them is a two- or three-way near tie
        q.mul_(4.0 / 1.5)
        k.mul_(4.0 / 1.5)
        grp = n // 16
        if grp:
            perm = torch.randperm(n, generator=g)
            lead, f1, f2 = perm[:grp], perm[grp:2 * grp], perm[2 * grp:2 * grp + (grp + 1) // 2]
            k[:, f1] = k[:, lead] + 0.05 * torch.randn(B, grp, H, HD, generator=g)
            k[:, f2] = k[:, lead[:f2.numel()]] + 0.05 * torch.randn(B, f2.numel(), H, HD, generator=g)
    elif name == "offset":
        # q and k without a component along e = (1, .., 1) / 8, then q += 8 e and a common vector +-200 e on every key: every scaled
        # logit of a row sits at +-200 + N(0, 2.25); exp overflows / underflows unless the row maximum is subtracted first
        e = torch.full((HD,), 0.125)
        for m in (q, k):
            m.sub_((m * e).sum(-1, keepdim=True) * e)
        q.add_(8.0 * e)
        sign = torch.tensor([1.0 if h % 2 == 0 else -1.0 for h in range(H)]).view(1, 1, H, 1)
        k.add_(200.0 * sign * e)
    elif name == "last_key":
        # key n-1 and one other key are near copies along a direction that every other query also points along: for those queries the
        # two share the top; v[n-1] stands out, so a dropped or doubled last key moves the output
        d = _unit(g, B, H)
        other = 0 if n <= 2 else n // 2
        k[:, n - 1:n] = 12.0 * d + 0.3 * torch.randn(B, 1, H, HD, generator=g)
        if n >= 2:
            k[:, other:other + 1] = 12.0 * d + 0.3 * torch.randn(B, 1, H, HD, generator=g)
        q[:, 0::2] += 12.0 * d
        v[:, n - 1] = 4.0
    elif name in ("ascending", "descending"):
        # scaled logit ~ +-4 per 64-key block along the sequence: the running maximum of the streaming kernel rises in every block
        # (ascending) or is fixed by the first block (descending)
        d = _unit(g, B, H)
        q.mul_(1.0 / 3.0).add_(8.0 * d)
        k.mul_(1.0 / 3.0)
        ramp = torch.arange(n, dtype=torch.float32).view(1, n, 1, 1) * (4.0 / BK)
        k.add_((ramp if name == "ascending" else -ramp) * d)
    else:
        raise ValueError(name)
    return x.reshape(B * n, 3 * H * HD).to(torch.bfloat16)


# ---- torch emulation of the kernels' arithmetic (optionally with a deliberate defect) -------------------------------------------------
def emulate(qkv, B, n, H, causal=False, streaming=False, ncon=0, defect=None):
    """fp32 scores, row maximum subtracted, exp2, P rounded to bf16, fp32 accumulation, bf16 output; the online form per 64-key block
    for the streaming kernel.  Returns (out bf16 [B*n, H*64], tap fp32 [B, H, ncon, n - ncon - 1] or None).
    defect: one of DEFECTS -- what a kernel with that bug would compute."""
    assert defect in (None,) + DEFECTS
    q, k, v = (t.float() for t in split(qkv, B, n, H))
    nk = n
    if defect == "dup_last":                                       # a padded key slot re-reads the last row and is not masked
        k = torch.cat([k, k[:, :, -1:]], dim=2)
        v = torch.cat([v, v[:, :, -1:]], dim=2)
        nk = n + 1
    c = torch.tensor(C, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    dead = torch.zeros(n, nk, dtype=torch.bool)
    if defect == "drop_last":
        dead[:, n - 1] = True
    if causal:
        shift = {"causal_plus": 1, "causal_minus": -1}.get(defect, 0)
        dead[:, :n] |= causal_mask(n, s.device, shift)
    s = torch.where(dead, torch.tensor(-1e30), s)
    if not streaming:
        m = s.max(-1, keepdim=True).values
        e = torch.exp2(s * c - m * c)
        l = e.sum(-1, keepdim=True)
        o = e.bfloat16().float() @ v
    else:
        m = torch.full(s.shape[:-1] + (1,), -1e30)
        l = torch.zeros_like(m)
        o = torch.zeros(s.shape[:-1] + (HD,))
        for j0 in range(0, nk, BK):
            sb = s[..., j0:j0 + BK]
            mn = torch.maximum(m, sb.max(-1, keepdim=True).values)
            a = torch.exp2((m - mn) * c)
            e = torch.exp2(sb * c - mn * c)
            l = l * a + e.sum(-1, keepdim=True)
            o = o * a + e.bfloat16().float() @ v[:, :, j0:j0 + BK]
            m = mn
        e = torch.exp2(s * c - m * c)                              # the tap's second pass, with the final maximum
    inv = 1.0 / l
    tap = None
    if ncon:
        tap = tapped((e * inv)[..., :n], ncon, 1 if defect == "tap_shift" else 0).contiguous()
    return merge(o * inv).bfloat16(), tap
