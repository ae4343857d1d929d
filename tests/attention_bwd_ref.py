"""Plain fp64 reference for the attention backward kernels (resident: attention_bwd.hip, streaming: attention_bwd_stream_kernel in
attention_stream.hip), with a DERIVED elementwise error bound for each of dq, dk, dv, seeded cotangent builders and a torch emulation
of either kernel's arithmetic.  The backward counterpart of tests/attention_ref.py, whose constants, helpers and qkv builders it imports.

Layout: qkv [B * ntok, 3 * heads * 64] bf16 (q | k | v), dO [B * ntok, heads * 64] bf16, dpext [B, heads, ncon, ntok - ncon - 1] fp32
(optional), dqkv [B * ntok, 3 * heads * 64] bf16 (dq | dk | dv), as the kernels.

The closed form (fp64, on the bf16-rounded inputs), one (image, head), n tokens, npatch = n - ncon - 1
=========================================================================================================
  P   = softmax(Q K^T / 8)
  dP  = dO V^T  (+ ext on query rows n - ncon .. n - 1, keys 1 .. npatch)
  D_q = sum_j P_qj dP_qj
  dS  = P o (dP - D) / 8
  dV  = P^T dO,   dQ = dS K,   dK = dS^T Q

The bound
=========
u, u32, gamma_n, c, EPS_EXP2 (2^-22 for the documented 1 ulp of v_exp_f32), tau = (1 + 2^-23)(1 + u32) - 1 as in attention_ref.py.
s = q . k (raw), S = sum_d |q_d| |k_d|, L = log2 sum_j exp2(s_j c) (so p_j = exp2(s_j c - L)), t_j = (s_j - max_i s_i) c,
G = sum_d |dO_d| |v_d|.  KP = keys padded to 32 (resident) / 64 (streaming), NB = KP / 64, NQ = 16 ceil(n / 16).

1. dP, both phases: two chained v_mfma_f32_16x16x32_bf16 (attention_bwd.hip:114-115, 245-246; attention_stream.hip:312-313, 449-450),
   then one fp32 addition where ext applies (attention_bwd.hip:121, 252; attention_stream.hip:319, 456):
       Delta_dP = gamma_64 G  [+ u32 (|dP| + gamma_64 G) on the ext pairs]
2. Phase-A weights w_j = Z p_j (1 + theta_j), Z common to the row, |theta_j| <= eps_j = expm1(x_j):
       x_j = gamma_64 S_j / 8                    the score MFMAs (attention_bwd.hip:105-106, attention_stream.hip:310-311)
           + ln2 u32 (2 c |s_j| + 2 |t_j|)       the fp32 constant scale_log2e (Z is fixed by L, so the constant no longer cancels: u32 c |s_j|),
                                                 the product and the subtraction (attention_bwd.hip:149, attention_stream.hip:350)
           + 2^-22                               v_exp_f32
   streaming, per later block (attention_stream.hip:342, 354-355): + ln2 3 u32 |t_j| + (NB - 1) 2^-22; alpha multiplies l and pd alike.
   sum / l: fp32 over n_acc = KP (+ 2 NB + 2 streaming: `l * alpha + bs` per block and the two shuffles) additions
   (attention_bwd.hip:151-154, attention_stream.hip:351-358):  sum = Z (1 + b), |b| <= beta = sum_j p_j ((1 + eps_j)(1 + gamma_nacc) - 1)
3. D_q = pd / sum (attention_bwd.hip:155-165: fp32 sum of the rounded products e_j dP_j over KP keys, `1.0f / sum`, `pd * inv`;
   attention_stream.hip:352-363: the same per block with `pd * alpha + bp`, one division), a_j = (1 + eps_j)(1 + gamma_(nacc + 1)) - 1:
       Delta_D = (sum_j p_j a_j |dP_j| + sum_j p_j (1 + a_j) Delta_dP_j + |D| beta) / (1 - beta) (1 + tau) + |D| tau
   (the forward bound's quotient with dP in the place of v).  D_q / 8 (attention_bwd.hip:168, attention_stream.hip:364) is exact.
4. lse = fl(mxs + v_log_f32(sum)) (attention_bwd.hip:168, attention_stream.hip:362; mxs is the very number subtracted in 2, it cancels):
       Delta_L = -log2(1 - beta)  +  2^-22 max(1, L - max_j s_j c)  +  u32 |L|
   the sum's error, v_log_f32 (1 ulp of a result in [0, log2 KP]), and the fp32 addition -- the term that scales with |lse| (offset builder).
5. Probabilities.  Resident phase A: e_j * inv (attention_bwd.hip:164, 173, 181):   epsA_j = (1 + eps_j)(1 + tau) / (1 - beta) - 1
   Phase B of both kernels and the streaming walk 2: exp2(s' c - lse) on a recomputed score (attention_bwd.hip:243-244, 260;
   attention_stream.hip:375, 447-448, 464):
       epsB_j = expm1(gamma_64 S_j / 8 + ln2 (u32 (2 c |s_j| + |s_j c - L|) + Delta_L) + 2^-22)
6. dS, rounded to bf16 as an MFMA operand (attention_bwd.hip:181-184, 271-272; attention_stream.hip:378-381, 475-476):
       phase A   w e (dP - D_q), w = inv / 8:  three fp32 roundings   R_A = (1 + epsA | epsB streaming)(1 + gamma_3)(1 + u) - 1
                 (streaming: 0.125 p (dP - D_q), attention_stream.hip:376: the same count)
       phase B   p fma(dP, 0.125, -D_q / 8):   two, fused or not      R_B = (1 + epsB)(1 + gamma_2)(1 + u) - 1
       E_dS = p / 8 (R |dP - D| + (1 + R)(Delta_dP + Delta_D))         absolute in dP and D: their cancellation needs no relative bound
7. Outputs, fp32 MFMA accumulation then bf16 (attention_bwd.hip:195, 202-203, 277-278, 286-289; attention_stream.hip:389, 396-397,
   481-482, 491-494); dQ sums KP keys, dK and dV sum NQ queries (rows past the sequence carry exactly 0):
       dQ:  E = (E_dS_A |K|)(1 + gamma_KP) + gamma_KP |dS| |K|          bound = E (1 + u) + u |dQ| + tiny
       dK:  E = (E_dS_B^T |Q|)(1 + gamma_NQ) + gamma_NQ |dS|^T |Q|      bound = E (1 + u) + u |dK| + tiny
       dV:  E = (P o ((1 + epsB)(1 + u)(1 + gamma_NQ) - 1))^T |dO|      bound = E (1 + u) + u |dV| + tiny     (P rounded to bf16:
            attention_bwd.hip:269-270, attention_stream.hip:473-474)
   tiny = 2^-100 n (1 + max |dP - D|) max(|q|, |k|, |dO|): exponentials that v_exp_f32 flushes to zero, subnormals.

To first order: u (sum |dS| |k| + |dQ|) and the like; every fp32 term is kept because the peaked and offset builders make
dP - D cancel and |lse| large.  Second-order products are covered as in attention_ref.py.
"""
import math

import torch

from attention_ref import (BK, C, EPS_EXP2, EPS_RCP, HD, TINY, U, U32, assert_within, build, gamma, merge, split,  # noqa: F401
                           _gen, B_TEST, H_TEST, BUILDERS, STREAM_BUILDERS, RESIDENT_LENGTHS, STREAM_LENGTHS, STREAM_MAX, STREAM_NCON,
                           TAP_NCON, TAP_BUILDERS, tap_lengths)

DO_BUILDERS = ("benign", "one_row", "scaled")
EXT_BUILDERS = ("benign", "corners")
CORNER = 1024.0
SCALED_LENGTHS = (17, 129, 288)
EDGE_LENGTHS = (35, 36, 37)               # n - 4 = 31, 32, 33: the shipped four concept tokens start just before / on / after a tile edge
STREAM_NCON_EDGE = (1, 15, 16, 17)
STREAM_NCON_LENGTHS = (129, 320)
DEFECTS = ("drop_last_key", "dup_last_key", "dup_last_query", "ext_phase_a_only", "ext_phase_b_only", "ext_key_shift", "ext_query_shift",
           "dq_from_o", "no_pd_rescale", "stale_block")
STREAM_ONLY_DEFECTS = ("no_pd_rescale", "stale_block")


def ext_lengths(ncon):
    return tuple(sorted(set(tap_lengths(ncon)) | (set(EDGE_LENGTHS) if ncon == 4 else set())))


def split_do(dO, B, n, H):
    """[B*n, H*64] -> [B, H, n, 64] fp64 (only the first B*n rows are looked at)"""
    return dO[:B * n].double().view(B, n, H, HD).permute(0, 2, 1, 3)


def _ext_full(dpext, B, n, H, ncon, like, qshift=0, kshift=0):
    """dpext scattered into [B, H, n, n]: rows n - ncon .. n - 1, keys 1 .. n - ncon - 1 (shifted for the emulation's defects)"""
    e = torch.zeros(B, H, n, n, dtype=like.dtype, device=like.device)
    if dpext is not None:
        np_ = n - ncon - 1
        e[:, :, n - ncon + qshift:n + qshift, 1 + kshift:1 + np_ + kshift] = dpext[:B].to(like.dtype).view(B, H, ncon, np_)
    return e


def closed_form(qkv, dO, dpext, B, n, H, ncon=0):
    """dq | dk | dv [B*n, 3*H*64] fp64 by the closed form of the module docstring"""
    q, k, v = split(qkv, B, n, H)
    g = split_do(dO, B, n, H)
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    dp = g @ v.transpose(-1, -2) + _ext_full(dpext, B, n, H, ncon, p)
    d = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - d) / 8.0
    return torch.cat([merge(ds @ k), merge(ds.transpose(-1, -2) @ q), merge(p.transpose(-1, -2) @ g)], dim=1)


def autograd(qkv, dO, dpext, B, n, H, ncon=0):
    """the same by fp64 autograd"""
    q, k, v = (t.clone().requires_grad_(True) for t in split(qkv, B, n, H))
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    loss = (merge(p @ v) * dO[:B * n].double()).sum()
    if dpext is not None:
        loss = loss + (p[:, :, n - ncon:, 1:n - ncon] * dpext.double()).sum()
    loss.backward()
    return torch.cat([merge(t.grad) for t in (q, k, v)], dim=1)


def bounds(qkv, dO, dpext, B, n, H, ncon=0, streaming=False):
    """(ref, bound), both [B*n, 3*H*64] fp64 (dq | dk | dv): the derivation of the module docstring, numbered as there"""
    q, k, v = split(qkv, B, n, H)
    g = split_do(dO, B, n, H)
    T = lambda x: x.transpose(-1, -2)
    s = q @ T(k)
    S = q.abs() @ T(k.abs())
    sc = s * C
    mx = sc.max(-1, keepdim=True).values
    L = mx + torch.log2(torch.exp2(sc - mx).sum(-1, keepdim=True))
    p = torch.exp2(sc - L)
    t = sc - mx
    blk = BK if streaming else 32
    KP = (n + blk - 1) // blk * blk
    NB = KP // BK
    NQ = (n + 15) // 16 * 16
    ln2 = math.log(2.0)
    tau = (1.0 + EPS_RCP) * (1.0 + U32) - 1.0
    # 1. dP
    ext = _ext_full(dpext, B, n, H, ncon, p)
    dp = g @ T(v) + ext
    d_dp = gamma(64) * (g.abs() @ T(v.abs()))
    if dpext is not None:
        on = torch.zeros(n, n, dtype=torch.bool, device=p.device)
        on[n - ncon:, 1:n - ncon] = True
        d_dp = torch.where(on, d_dp + U32 * (dp.abs() + d_dp), d_dp)
    # 2. phase-A weights and their sum
    x = gamma(64) * S / 8.0 + ln2 * U32 * (2.0 * sc.abs() + 2.0 * t.abs()) + EPS_EXP2
    nacc = KP
    if streaming:
        x = x + ln2 * 3.0 * U32 * t.abs() + (NB - 1) * EPS_EXP2
        nacc = KP + 2 * NB + 2
    eps = torch.expm1(x)
    beta = (p * ((1.0 + eps) * (1.0 + gamma(nacc)) - 1.0)).sum(-1, keepdim=True)
    # 3. D_q
    d = (p * dp).sum(-1, keepdim=True)
    a = (1.0 + eps) * (1.0 + gamma(nacc + 1)) - 1.0
    d_d = ((p * a * dp.abs()).sum(-1, keepdim=True) + (p * (1.0 + a) * d_dp).sum(-1, keepdim=True) + d.abs() * beta) / (1.0 - beta) * (1.0 + tau) \
        + d.abs() * tau
    # 4. lse
    d_l = -torch.log2(1.0 - beta) + EPS_EXP2 * (L - mx).clamp_min(1.0) + U32 * L.abs()
    # 5. probabilities
    eps_a = (1.0 + eps) * (1.0 + tau) / (1.0 - beta) - 1.0
    eps_b = torch.expm1(gamma(64) * S / 8.0 + ln2 * (U32 * (2.0 * sc.abs() + (sc - L).abs()) + d_l) + EPS_EXP2)
    # 6. dS
    ds = p * (dp - d) / 8.0
    r_a = (1.0 + (eps_b if streaming else eps_a)) * (1.0 + gamma(3)) * (1.0 + U) - 1.0
    r_b = (1.0 + eps_b) * (1.0 + gamma(2)) * (1.0 + U) - 1.0
    e_ds = lambda r: p / 8.0 * (r * (dp - d).abs() + (1.0 + r) * (d_dp + d_d))
    # 7. outputs
    tiny = TINY * n * (1.0 + float((dp - d).abs().max())) * max(float(q.abs().max()), float(k.abs().max()), float(g.abs().max()))
    dq, dk, dv = ds @ k, T(ds) @ q, T(p) @ g
    eq = (e_ds(r_a) @ k.abs()) * (1.0 + gamma(KP)) + gamma(KP) * (ds.abs() @ k.abs())
    ek = (T(e_ds(r_b)) @ q.abs()) * (1.0 + gamma(NQ)) + gamma(NQ) * (T(ds.abs()) @ q.abs())
    ev = T(p * ((1.0 + eps_b) * (1.0 + U) * (1.0 + gamma(NQ)) - 1.0)) @ g.abs()
    ref = torch.cat([merge(dq), merge(dk), merge(dv)], dim=1)
    bound = torch.cat([merge(e * (1.0 + U) + U * o.abs() + tiny) for e, o in ((eq, dq), (ek, dk), (ev, dv))], dim=1)
    return ref, bound


def assert_all_within(got, ref, bound, what):
    """attention_ref.assert_within on each of dq, dk, dv; returns the three worst error / bound ratios"""
    D = ref.shape[1] // 3
    return tuple(assert_within(got[:, i * D:(i + 1) * D], ref[:, i * D:(i + 1) * D], bound[:, i * D:(i + 1) * D], f"{what} {nm}")
                 for i, nm in enumerate(("dq", "dk", "dv")))


# ---- seeded cotangents: CPU generator, the same bytes on every machine -------------------------------------------------------------
def build_do(name, B, n, H, seed=0):
    """dO [B*n, H*64] bf16 on the CPU"""
    g = _gen("dO/" + name, n, seed)
    x = torch.randn(B, n, H * HD, generator=g)
    if name == "benign":
        pass
    elif name == "one_row":
        # one non-zero query row per image: the last token (even images), token 0 (odd images) -- any other row's dS, and every
        # contribution of another row to dK / dV, is exactly zero, so row cross-talk shows
        keep = torch.zeros(B, n, 1)
        for b in range(B):
            keep[b, n - 1 if b % 2 == 0 else 0] = 1.0
        x = x * keep
    elif name == "scaled":
        # per-row magnitudes 2^-6 .. 2^6 (a seeded permutation of an even spread of exponents)
        ex = torch.linspace(-6.0, 6.0, B * n)[torch.randperm(B * n, generator=g)].view(B, n, 1)
        x = x * torch.exp2(ex)
    else:
        raise ValueError(name)
    return x.reshape(B * n, H * HD).to(torch.bfloat16)


def build_ext(name, B, n, H, ncon, seed=0):
    """dpext [B, H, ncon, n - ncon - 1] fp32 on the CPU"""
    np_ = n - ncon - 1
    assert ncon >= 1 and np_ >= 1
    g = _gen(f"ext/{name}/{ncon}", n, seed)
    if name == "benign":
        return 3.0 * torch.randn(B, H, ncon, np_, generator=g)
    if name == "corners":
        # zero but for +-CORNER at (first | last concept row) x (key 1 | key npatch): 1024 against |dP - D| of order 10 moves dS of that
        # pair by p CORNER / 8, a thousand times the bf16 rounding of the row's other terms for p ~ 1 / n, so an entry dropped or
        # applied one row / one key off breaches the bound (tests/test_attention_bwd_ref_cpu.py shows it)
        e = torch.zeros(B, H, ncon, np_)
        e[:, :, 0, 0] = CORNER                                     # assigned, not added: corners that coincide (ncon = 1, npatch = 1) stay large
        e[:, :, 0, np_ - 1] = -CORNER
        e[:, :, ncon - 1, 0] = -CORNER
        e[:, :, ncon - 1, np_ - 1] = CORNER
        return e
    raise ValueError(name)


# ---- torch emulation of the kernels' arithmetic (optionally with a deliberate defect) -------------------------------------------------
def emulate(qkv, dO, dpext, B, n, H, ncon=0, streaming=False, defect=None):
    """fp32 scores and dP, fp32 statistics (block-wise with alpha for the streaming kernel), dS by the phase-A formula for dQ and by
    the phase-B formula for dK, P and dS rounded to bf16, fp32 accumulation, bf16 outputs.  Returns dq | dk | dv [B*n, 3*H*64] bf16.
    defect: one of DEFECTS -- what a kernel with that bug would compute."""
    assert defect in (None,) + DEFECTS
    assert streaming or defect not in STREAM_ONLY_DEFECTS
    q, k, v = (t.float() for t in split(qkv, B, n, H))
    g = split_do(dO, B, n, H).float()
    T = lambda x: x.transpose(-1, -2)
    bf = lambda x: x.bfloat16().float()
    c = torch.tensor(C, dtype=torch.float32)
    s = q @ T(k)
    dp0 = g @ T(v)
    ka = k                                                         # phase A's keys
    if defect == "dup_last_key":                                   # a padded key slot re-reads the last row and is not masked in phase A
        s_a = torch.cat([s, s[..., -1:]], dim=-1)
        dp_a = torch.cat([dp0, dp0[..., -1:]], dim=-1)
        ka = torch.cat([k, k[:, :, -1:]], dim=2)
    else:
        s_a, dp_a = s.clone(), dp0.clone()
    if defect == "drop_last_key":
        s_a[..., n - 1] = -1e30
    ext = lambda **kw: _ext_full(dpext, B, n, H, ncon, s, **kw)
    shift = dict(kshift=-1) if defect == "ext_key_shift" else dict(qshift=-1) if defect == "ext_query_shift" else {}
    e_a = ext(**shift) if defect != "ext_phase_b_only" else torch.zeros_like(s)
    e_b = ext(**shift) if defect != "ext_phase_a_only" else torch.zeros_like(s)
    dp_d = dp_a.clone() if defect == "dq_from_o" else dp_a         # what D_q is summed over: dO . O lacks the ext term
    dp_a[..., :n] += e_a
    dp_b = dp0 + e_b
    nk = s_a.shape[-1]
    # ---- phase A: statistics
    if not streaming:
        mxs = s_a.max(-1, keepdim=True).values * c
        e = torch.exp2(s_a * c - mxs)
        l = e.sum(-1, keepdim=True)
        pd = (e * dp_d).sum(-1, keepdim=True)
        inv = 1.0 / l
        dq_ = pd * inv
        lse = mxs + torch.log2(l)
        ds_a = (0.125 * inv) * e * (dp_a - dq_)
    else:
        m = torch.full(s.shape[:-1] + (1,), -1e30)
        l = torch.zeros_like(m)
        pd = torch.zeros_like(m)
        for j0 in range(0, nk, BK):
            sb, db = s_a[..., j0:j0 + BK], dp_d[..., j0:j0 + BK]
            if defect == "stale_block" and j0 == 2 * BK:           # the ring stage still holds the block staged two steps earlier
                w = sb.shape[-1]
                sb, db = s_a[..., :w], dp_a[..., :w]
            mn = torch.maximum(m, sb.max(-1, keepdim=True).values)
            al = torch.exp2((m - mn) * c)
            e = torch.exp2(sb * c - mn * c)
            l = l * al + e.sum(-1, keepdim=True)
            pd = (pd if defect == "no_pd_rescale" else pd * al) + (e * db).sum(-1, keepdim=True)
            m = mn
        lse = m * c + torch.log2(l)
        dq_ = pd / l
        ds_a = 0.125 * torch.exp2(s_a * c - lse) * (dp_a - dq_)
    dq = bf(ds_a) @ ka
    # ---- phase B: P and dS rebuilt from (lse, D_q / 8)
    qb, gb, sb_, dpb, lse_b, d8 = q, g, s, dp_b, lse, 0.125 * dq_
    if defect == "dup_last_query":                                 # a query row past the sequence (a re-read of the last one) keeps its real statistics
        dup = lambda x: torch.cat([x, x[:, :, -1:]], dim=2)
        qb, gb, sb_, dpb, lse_b, d8 = dup(q), dup(g), dup(s), dup(dp_b), dup(lse), dup(d8)
    p_b = torch.exp2(sb_ * c - lse_b)
    ds_b = p_b * (dpb * 0.125 - d8)
    dk = T(bf(ds_b)) @ qb
    dv = T(bf(p_b)) @ gb
    return torch.cat([merge(dq), merge(dk), merge(dv)], dim=1).bfloat16()
