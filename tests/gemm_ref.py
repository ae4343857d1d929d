"""fp64 references, derived error bounds and a rounding-faithful CPU emulation of the ten FORWARD epilogues of the bf16 GEMM family
(csrc/gemm_epilogue.h::store_tile behind gemm_bf16.hip, gemm_pp.hip, gemm_r4.hip; kernels.h EPI_*):

    0 bias | 1 bias + quick_gelu | 2 bias + gelu | 3 bias + residual (+ bf16 copy) | 4 scale + residual (+ addend)
    6 bias + row statistics | 7 = 4 + bf16 copy + its row statistics | 8 / 9 / 10 LayerNorm-folded linear (+ quick_gelu / gelu)

Plain torch on fp64; every function runs on CPU or GPU tensors alike.  tests/test_gemm_ref_cpu.py proves on the CPU that the clean
emulation stays inside every bound and that each listed defect leaves one; tests/test_gemm_fwd_epilogues_gpu.py holds the kernels to the
same bounds.

Notation.  X [M, K], W [N, K] are bf16 and enter exactly.  u = 2^-8 (one bf16 rounding, round to nearest even), u32 = 2^-24 (one fp32
rounding), gamma_n = n u32 / (1 - n u32).  Z = X W^T and A = |X| |W|^T in fp64.  TINY = 2^-126 is added to every bound: a result below
the smallest normal number may be flushed to zero, and a bound of exactly zero would test nothing.

The accumulator.  A product of two bf16 numbers has 16 significant bits and is exact in fp32; the MFMA chain adds K such products into
an fp32 accumulator, so |acc - Z| <= gamma_K A whatever the order of the K - 1 additions (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2).  A split-K launch adds the same K terms (K / S per slice, then S slabs in slice order): gamma_K is unchanged.

Plain (0, 1, 2), want = act(Z + b).  `acc + bias[nt]` rounds once:
    e_pre = (1 + u32) gamma_K A + u32 |pre|,            pre = Z + b.
The activation moves that by at most its Lipschitz constant L = sup |act'|: 1 for the identity; 1.10 for quick_gelu, whose derivative
s (1 + 1.702 x (1 - s)), s = sigmoid(1.702 x), peaks at 1.0998 (x = 1.41) and bottoms at -0.0998; 1.13 for gelu, whose derivative
Phi(x) + x phi(x) peaks at 1.1289 (x = sqrt 2) and bottoms at -0.1289 (test_gemm_ref_cpu.py re-measures both).  The kernel's formula
(quick_gelu_f / gelu_erf_f: exp2 and rcp instructions, erf by Abramowitz & Stegun 7.1.26) differs from the exact function by at most
delta_act in absolute terms -- `_deltas()`: the fp32 formulas on the CPU against fp64 over every bf16 |x| <= 256; past 256 both
formulas return x or (-)0 exactly.  The instructions' own error (1 ulp each on the hardware, none on the CPU) is relative, at most
8 u32 |act|, and fits in the gap between u and the true worst relative error of a bf16 rounding, u / (1 + u).  Then the output rounds:
    |got - want| <= (1 + u) (L e_pre + delta_act) + u |want|.

Residual (3, 4, 7), in fp32, want = h + [addend] + s (Z + b) with s the fp32 scale (1 for epilogue 3).  One u32 per operation
store_tile performs, each on the magnitude it rounds (a fused multiply-add only removes one of them):
    v = acc + bias             e_v = (1 + u32) gamma_K A + u32 |Z + b|
    t = v * s                  e_t = (1 + u32) |s| e_v + u32 |s (Z + b)|              (4, 7 only)
    r = h + t                  e_r = (1 + u32) e_t + u32 |h + s (Z + b)|
    r' = r + addend            e   = (1 + u32) e_r + u32 |want|                       (with an addend only: + 0.0f is exact)
The bf16 copy of epilogue 3 is bf16(v): against Z + b it is a plain epilogue (L = 1, delta = 0); with h = 0 the residual comes back as
v itself, and the copy must be its rounding bit for bit.  hb_out of epilogue 7 must equal bf16(resid_got) bit for bit.

Statistics (6, 7).  Each (sum, sum of squares) partial is checked against the fp64 sums of the kernel's OWN 64 rounded outputs x_j.
Any summation of 64 numbers makes 63 additions, so |sum - sum_j x_j| <= gamma_63 sum |x_j| <= gamma_64 sum |x_j| in any order; the
squares of bf16 numbers are exact in fp32 and the same 63 additions follow, gamma_65 sum x_j^2 with room for one rounded product each.
Those two are the bounds of record.  The trees are far shallower: epilogue 6 adds pairs, four pairs per lane, then sum8's three DPP
steps (1 + 3 + 3 = 7 roundings on any path); epilogue 7 adds (a + b) + (c + d) per lane and sum16's four steps (2 + 4 = 6).  A value
passes through at most 7 additions, so gamma_7 sum |x_j| holds too (Higham section 4.2, pairwise summation): `bound_tree`, asserted
next to the bounds of record, which it undercuts by 9x -- the slack of the order-free figure, not of the kernel.

Fold (8, 9, 10).  The reference is the exact function of the kernel's inputs, the fp32 partials included; it is NOT a LayerNorm of
unfolded weights.  With p = K / 64 partials (s_i, q_i) per row, c = fold_c, d = bias:
    mean = sum s_i / K,  var = sum q_i / K - mean^2,  rstd = (max(var, 0) + eps)^-1/2,  y = rstd (X W'^T - mean c) + d.
  * fold_stats_finish sums the p partials in fp32 (pairs, then two strided halves, then the other lane), multiplies by the rounded
    1 / K:  e_mean = gamma_(p + 2) sum |s_i| / K, and likewise gamma_(p + 2) sum |q_i| / K on sq / K.
  * the cancellation  sq / K - mean * mean:  e_var = (1 + u32) (gamma_(p + 2) sum |q_i| / K + 2 |mean| e_mean + e_mean^2 + u32 mean^2)
    + u32 |var|;  max(., 0) is 1-Lipschitz;  adding eps rounds once: e_ve = (1 + u32) e_var + u32 (var + eps).
  * x^-1/2 at x >= ve - e_ve: relative error rho = (1 - e_ve / ve)^-1/2 - 1 (to first order e_var / (2 (var + eps))), infinite --
    the input tests nothing -- where e_ve >= ve; times rsqrtf's own error.  No accuracy table of the device math library is
    installed next to the compiler; 2 ulp (2 * 2^-23 relative) is ASSUMED, three orders of magnitude below the other terms.
  * store_tile: pre = acc * rs + (c * nm + d), nm = -mean * rs.  The same rs multiplies both parts, so its error scales the
    DIFFERENCE:  rho rstd |Z - mean c|;  the rounded factors carry (1 + rho) rstd (gamma_K A + |c| e_mean);  the roundings: two on
    acc * rs, four on c * mean * rs, two on d -- gamma_3 |Z|, gamma_5 |c mean| (times (1 + rho) rstd) and gamma_3 |d| with room.
  e_pre is their sum; activation and output rounding as for the plain epilogues.
For a constant row (var = 0) only eps keeps rstd finite and the cancellation term is of the order of eps itself; for a row whose
mean is 1e3 deviations the bound on that row is tens of percent.  That is the true worst case of the fp32 statistics, not slack.

Emulation.  `emulate` restates each epilogue in fp32 / bf16 on the CPU: fp32 accumulation in 64-wide K-tile order (slice by slice for
split-K), a rounding wherever the kernel rounds, the kernel's own activation formulas.  `DEFECTS` lists the mistakes the bounds must
catch; `addend_ldr` only shows where ldr != ld_addend, `splitk_drop_slice` only in a split launch, and no output-level test can see a
defect that permutes the partials a fold consumer reads, because it sums them all.
"""
import math

import torch

U = 2.0 ** -8
U32 = 2.0 ** -24
TINY = 2.0 ** -126
RSQRT_ULPS = 2                            # assumed (module docstring)
EPI_BIAS, EPI_QUICK, EPI_GELU, EPI_BIAS_RESID, EPI_SCALE_RESID = range(5)
EPI_BIAS_STATS, EPI_SCALE_RESID_STATS, EPI_FOLD_BIAS, EPI_FOLD_QUICK, EPI_FOLD_GELU = 6, 7, 8, 9, 10
FORWARD = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)
FOLD = (8, 9, 10)
ACT = {0: None, 1: "quick", 2: "gelu", 3: None, 6: None, 8: None, 9: "quick", 10: "gelu"}
LIPSCHITZ = {None: 1.0, "quick": 1.10, "gelu": 1.13}
SPECIAL = (0.0, -0.0, 8.0, -8.0, 30.0, -30.0, 88.0, -88.0, 1e4, -1e4)
SPECIAL_COLS = (0, 9, 18, 27, 36, 45, 54, 63, 70, 127)         # every 16-byte chunk position of a 64-column slice, both slices
DEFECTS = ("drop_last_ktile", "bias_col_plus_1", "no_eps", "stats_next_slice", "scale_on_addend", "stats_unrounded", "addend_ldr",
           "splitk_drop_slice", "act_before_bias")


def gamma(n):
    return n * U32 / (1.0 - n * U32)


# ---- exact activations / derivatives (fp64) and the kernels' formulas (fp32, CPU) -----------------------------------------------------
def _quick(x):
    return x * torch.sigmoid(1.702 * x)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _dquick(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1.0 + 1.702 * x * (1.0 - s))


def _dgelu(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _kernel_formulas(x):
    """gemm_epilogue.h in fp32: (dquick_gelu_f, dgelu_erf_f, quick_gelu_f, gelu_erf_f)(x)"""
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    exp2, rcp = torch.exp2, torch.reciprocal
    s = rcp(1.0 + exp2(f(-2.4554669595930157) * x))
    dquick = s * (1.0 + f(1.702) * x * (1.0 - s))
    quick = x * s
    z = x.abs() * f(0.70710678118654752)
    t = rcp(1.0 + f(0.3275911) * z)
    poly = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
    e = exp2(f(-1.4426950408889634) * z * z)
    erf_abs = 1.0 - poly * e
    cdf = 0.5 * (1.0 + torch.copysign(erf_abs, x))
    dgelu = cdf + x * f(0.3989422804014327) * e
    gelu = 0.5 * x * (1.0 + torch.copysign(erf_abs, x))
    return dquick, dgelu, quick, gelu


_DELTAS = {}


def _deltas():
    """{'dquick', 'dgelu'} over every bf16 |x| <= 1e4, {'quick', 'gelu'} over every bf16 |x| <= 256"""
    if not _DELTAS:
        bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
        x = bits.view(torch.bfloat16).float()
        x = x[torch.isfinite(x) & (x.abs() <= 1e4)]
        exact = [f(x.double()) for f in (_dquick, _dgelu, _quick, _gelu)]
        worst = [0.0] * 4
        got = _kernel_formulas(x)
        for i in range(4):
            sel = slice(None) if i < 2 else (x.abs() <= 256)
            worst[i] = float((got[i].double() - exact[i])[sel].abs().max())
        _DELTAS.update(dquick=worst[0], dgelu=worst[1], quick=worst[2], gelu=worst[3])
        print("deltas (fp32 formulas vs fp64): " + ", ".join(f"{k} {v:.2e}" for k, v in _DELTAS.items()))
    return _DELTAS


def act64(name, x):
    return x if name is None else (_quick if name == "quick" else _gelu)(x)


def act32(name, x):
    """the kernel's formula on fp32 CPU values"""
    return x if name is None else _kernel_formulas(x)[2 if name == "quick" else 3]


def delta_act(name):
    return 0.0 if name is None else _deltas()[name]


def act_bound(name, x64):
    """want, bound of a fused activation whose fp32 input IS x (no pre-activation error): u |act(x)| + delta_act"""
    want = act64(name, x64)
    return want, U * want.abs() + delta_act(name) + TINY


# ---- operands -----------------------------------------------------------------------------------------------------------------------
class Ops:
    """The operands of one launch, valid rows only: X [M, K], W [N, K] bf16; bias [N] fp32; h [M, N] fp32; addend [M, N] bf16 or None;
    scale: a Python float that is an fp32 number; stats [M, K / 64, 2], fold_c [N] fp32 and eps (an fp32 number) for the fold."""

    def __init__(self, X, W, bias, h=None, addend=None, scale=None, stats=None, fold_c=None, eps=None):
        self.X, self.W, self.bias, self.h, self.addend, self.scale = X, W, bias, h, addend, scale
        self.stats, self.fold_c, self.eps = stats, fold_c, eps
        self.M, self.K = X.shape
        self.N = W.shape[0]
        self._cache, self._cpu = {}, {}

    def cpu(self):
        mv = lambda t: None if t is None else t.cpu()
        return Ops(mv(self.X), mv(self.W), mv(self.bias), mv(self.h), mv(self.addend), self.scale, mv(self.stats), mv(self.fold_c), self.eps)

    def products(self):
        if "ZA" not in self._cache:
            Xd, Wd = self.X.double(), self.W.double()
            self._cache["ZA"] = (Xd @ Wd.t(), Xd.abs() @ Wd.abs().t())
        return self._cache["ZA"]


def operands(M, N, K, seed, device="cuda"):
    """The operands of tests/test_gemm_train_epilogues_gpu.py: X padded with zero rows to a multiple of 256"""
    g = torch.Generator(device=device).manual_seed(seed)
    Mp = (M + 255) // 256 * 256
    X = torch.zeros(Mp, K, dtype=torch.bfloat16, device=device)
    X[:M] = torch.randn(M, K, generator=g, device=device).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device=device) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g, device=device)
    return g, Mp, X, W, bias


def slice_stats(x_bf16):
    """[M, K] bf16 -> fp32 [M, K / 64, 2]: (sum, sum of squares) of every 64-column slice, summed in fp64 and rounded once"""
    xs = x_bf16.double().view(x_bf16.shape[0], -1, 64)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).float()


def fold_operands(M, N, K, device="cuda"):
    """The LayerNorm-folded operands of tests/test_gemm_gpu.py::test_layernorm_folded_consumers: X, W' = bf16(W gamma), d, c, the
    partials of X, and the LayerNorm of the UNFOLDED weights in fp64 (the looser, algebraic reference)"""
    g = torch.Generator(device=device).manual_seed(5)
    Mp = (M + 255) // 256 * 256
    x = torch.randn(M, K, generator=g, device=device) * (0.5 + 3 * torch.rand(M, 1, generator=g, device=device)) \
        + 2 * torch.randn(M, 1, generator=g, device=device)
    x[:, 5] *= 20
    X = torch.zeros(Mp, K, dtype=torch.bfloat16, device=device)
    X[:M] = x.to(torch.bfloat16)
    W32 = torch.randn(N, K, generator=g, device=device) * K ** -0.5
    gam = 1 + 0.3 * torch.randn(K, generator=g, device=device)
    beta = 0.2 * torch.randn(K, generator=g, device=device)
    b = torch.randn(N, generator=g, device=device)
    Wf = (W32 * gam).to(torch.bfloat16)
    c = Wf.float().sum(1)
    d = b + W32 @ beta
    stats = torch.zeros(Mp, K // 64, 2, device=device)
    xs = X[:M].double().view(M, -1, 64)
    stats[:M] = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).float()
    xn = torch.nn.functional.layer_norm(X[:M].double(), (K,), gam.double(), beta.double(), 1e-5)
    pre = xn @ W32.double().t() + b.double()
    assert float(pre.abs().max()) < 256.0                                   # the range delta_act was measured over
    return X, Wf, d, c, stats, pre


def fwd_case(M, N, K, device="cuda"):
    """`operands` with the SPECIAL values written into the pre-activation: column col of W is zeroed and its bias set, so Z + b is that
    value exactly in every row; a residual, a bf16 addend and a scale for the read-modify-write epilogues"""
    g, _, X, W, bias = operands(M, N, K, 31, device)
    for col, val in zip(SPECIAL_COLS, SPECIAL):
        W[col] = 0
        bias[col] = val
    h = torch.randn(M, N, generator=g, device=device)
    addend = torch.randn(M, N, generator=g, device=device).to(torch.bfloat16)
    return Ops(X[:M].clone(), W, bias, h=h, addend=addend, scale=float(torch.tensor(0.37, dtype=torch.float32)))


def fold_case(M, N, K, device="cuda"):
    """`fold_operands` plus, from three rows up, one constant row (var = 0: only eps keeps rstd finite) and one row of 1.0 with every 64th
    element one bf16 step higher (mean = 1032 deviations); the SPECIAL values enter through d with the weight row and c zeroed"""
    X, Wf, d, c, stats, _ = fold_operands(M, N, K, device)
    X = X[:M].clone()
    if M >= 3:
        X[M - 2] = 0.5
        X[M - 1] = 1.0
        X[M - 1, 7::64] = 1.0 + 2.0 ** -7
    for col, val in zip(SPECIAL_COLS, SPECIAL):
        Wf[col] = 0
        c[col] = 0
        d[col] = val
    return Ops(X, Wf, d, stats=slice_stats(X), fold_c=c, eps=float(torch.tensor(1e-5, dtype=torch.float32)))


# ---- references and bounds ----------------------------------------------------------------------------------------------------------
def _finish(name, pre, e_pre):
    want = act64(name, pre)
    e1 = LIPSCHITZ[name] * e_pre + delta_act(name)
    return want, (1.0 + U) * e1 + U * want.abs() + TINY


def _affine(o):
    """Z + b, and the error of the kernel's v = acc + bias"""
    Z, A = o.products()
    z = Z + o.bias.double()
    return z, (1.0 + U32) * gamma(o.K) * A + U32 * z.abs()


def out_ref(epi, o):
    """(want, bound) of the bf16 output of epilogues 0, 1, 2, 3, 6 (against fp64) and 8, 9, 10"""
    key = ("out", ACT[epi], epi in FOLD)
    if key not in o._cache:
        o._cache[key] = _fold_ref(ACT[epi], o) if epi in FOLD else _finish(ACT[epi], *_affine(o))
    return o._cache[key]


def resid_ref(epi, o, with_addend=True, zero_h=False):
    """(want, bound) of the fp32 residual of epilogues 3, 4, 7"""
    key = ("resid", epi == EPI_BIAS_RESID, with_addend, zero_h)
    if key not in o._cache:
        o._cache[key] = _resid_ref(epi, o, with_addend, zero_h)
    return o._cache[key]


def _resid_ref(epi, o, with_addend, zero_h):
    z, e_v = _affine(o)
    h = torch.zeros_like(z) if zero_h else o.h.double()
    if epi == EPI_BIAS_RESID:
        want = h + z
        return want, (1.0 + U32) * e_v + U32 * want.abs() + TINY
    s = float(o.scale)
    t = s * z
    e_t = (1.0 + U32) * abs(s) * e_v + U32 * t.abs()
    r = h + t
    e_r = (1.0 + U32) * e_t + U32 * r.abs()
    if not with_addend:
        return r, e_r + TINY
    want = r + o.addend.double()
    return want, (1.0 + U32) * e_r + U32 * want.abs() + TINY


def stats_ref(x):
    """x [M, N]: the kernel's own rounded outputs -> (want [M, N / 64, 2], bound of record, bound of the trees)"""
    xs = x.double().view(x.shape[0], -1, 64)
    sa, q = xs.abs().sum(-1), (xs * xs).sum(-1)
    want = torch.stack([xs.sum(-1), q], dim=-1)
    return want, torch.stack([gamma(64) * sa, gamma(65) * q], dim=-1) + TINY, torch.stack([gamma(7) * sa, gamma(7) * q], dim=-1) + TINY


def fold_stats64(o):
    """(mean, var, rstd, e_mean, rho) per row, fp64 (module docstring)"""
    st = o.stats.double()
    p, K = st.shape[1], float(o.K)
    g = gamma(p + 2)
    mean = st[..., 0].sum(-1) / K
    var = st[..., 1].sum(-1) / K - mean * mean
    ve = var.clamp_min(0.0) + o.eps
    rstd = ve.rsqrt()
    e_mean = g * st[..., 0].abs().sum(-1) / K
    e_var = (1.0 + U32) * (g * st[..., 1].abs().sum(-1) / K + 2.0 * mean.abs() * e_mean + e_mean * e_mean + U32 * mean * mean) + U32 * var.abs()
    frac = ((1.0 + U32) * e_var + U32 * ve) / ve
    rho = torch.where(frac < 1.0, (1.0 - frac.clamp_max(0.999999)).rsqrt() - 1.0, torch.full_like(frac, float("inf")))
    rho = (1.0 + rho) * (1.0 + RSQRT_ULPS * 2.0 ** -23) - 1.0
    return mean, var, rstd, e_mean, rho


def _fold_ref(name, o):
    Z, A = o.products()
    mean, _, rstd, e_mean, rho = (t[:, None] for t in fold_stats64(o))
    c, d = o.fold_c.double()[None, :], o.bias.double()[None, :]
    Zc = Z - mean * c
    pre = rstd * Zc + d
    e_pre = (1.0 + rho) * rstd * (gamma(o.K) * A + c.abs() * e_mean + gamma(3) * Z.abs() + gamma(5) * c.abs() * (mean.abs() + e_mean)) \
        + gamma(3) * d.abs() + rho * rstd * Zc.abs()
    return _finish(name, pre, e_pre)


# ---- what a launch of epilogue `epi` must satisfy -----------------------------------------------------------------------------------
def checks(epi, o, got, with_addend=True, zero_h=False):
    """got: CPU tensors {'out' bf16, 'resid' fp32, 'hb' bf16, 'stats' fp32} of the valid rows and columns, as the epilogue has them.
    Returns [("bound", group, name, got, want, bound) | ("equal", group, name, a, b)] with everything on the CPU."""
    def cpu(t):                                                               # one copy per reference, however many launches use it
        if id(t) not in o._cpu:
            o._cpu[id(t)] = (t, t.cpu())
        return o._cpu[id(t)][1]
    res = []
    if epi in (0, 1, 2, 3, 6) or epi in FOLD:
        want, bound = out_ref(epi, o)
        group = "fold" if epi in FOLD else "plain"
        res.append(("bound", group, "out", got["out"], cpu(want), cpu(bound)))
    if epi in (3, 4, 7):
        want, bound = resid_ref(epi, o, with_addend, zero_h)
        res.append(("bound", "residual", "resid", got["resid"], cpu(want), cpu(bound)))
    if epi == 3 and zero_h:
        res.append(("equal", "residual", "out == bf16(resid)", got["out"].view(torch.int16), got["resid"].to(torch.bfloat16).view(torch.int16)))
    if epi == 7:
        res.append(("equal", "residual", "hb == bf16(resid)", got["hb"].view(torch.int16), got["resid"].to(torch.bfloat16).view(torch.int16)))
    if epi in (6, 7):
        want, bound, tree = stats_ref(got["out"] if epi == 6 else got["hb"])
        res.append(("bound", "stats", "stats", got["stats"], want, bound))
        res.append(("bound", "stats tree", "stats", got["stats"], want, tree))
    return res


def failed(res):
    """the names of the checks of `checks` that do not hold"""
    bad = []
    for r in res:
        if r[0] == "equal":
            ok = r[3].shape == r[4].shape and bool(torch.equal(r[3], r[4]))
        else:
            g = r[3].double()
            ok = g.shape == r[4].shape and bool(torch.isfinite(g).all()) and bool(torch.isfinite(r[5]).all()) and not bool(((g - r[4]).abs() > r[5]).any())
        if not ok:
            bad.append(f"{r[1]}: {r[2]}")
    return bad


# ---- the emulation ------------------------------------------------------------------------------------------------------------------
def _accumulate(o, defect, split):
    """fp32 accumulation of 64-wide K-tiles in order; split > 1: K / split columns per slice, the slabs added in slice order"""
    Xf, Wf = o.X.float(), o.W.float()
    tiles = [(k, min(k + 64, o.K)) for k in range(0, o.K, 64)]
    if defect == "drop_last_ktile":
        tiles = tiles[:-1]
    per = len(tiles) if split == 1 else o.K // split // 64
    acc = torch.zeros(o.M, o.N)
    for s in range(0, len(tiles), max(per, 1)):
        if split > 1 and defect == "splitk_drop_slice" and s == per:          # slice 1 never reaches the sum
            continue
        slab = torch.zeros(o.M, o.N)
        for k0, k1 in tiles[s:s + per]:
            slab = slab + Xf[:, k0:k1] @ Wf[:, k0:k1].t()
        acc = acc + slab if split > 1 else slab
    return acc


def _stats32(x, defect):
    """(sum, sum of squares) per 64-column slice in fp32; `stats_next_slice`: slot j holds the statistics of slice j + 1"""
    xs = x.view(x.shape[0], -1, 64)
    st = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1)
    return torch.roll(st, -1, dims=1) if defect == "stats_next_slice" else st


def emulate(epi, o, defect=None, split=1, with_addend=True, zero_h=False, ldr=None, ld_addend=None):
    """Epilogue `epi` of CPU operands `o` in the kernel's arithmetic -> the dict `checks` takes.  ldr / ld_addend: the leading
    dimensions of the launch (only `addend_ldr` reads them; gaps hold NaN as in the GPU test)."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    name = ACT.get(epi)
    acc = _accumulate(o, defect, split)
    bias = o.bias.roll(-1) if defect == "bias_col_plus_1" else o.bias
    if epi in FOLD:
        st = o.stats
        n4 = o.K // 128
        H = (n4 + 1) // 2
        halves = []
        for half in (0, 1):                                                   # fold_stats_finish: two lanes per row, H float4s each
            sm, sq = torch.zeros(o.M), torch.zeros(o.M)
            for i in range(H):
                j = half * H + i
                if j < n4:
                    sm = sm + (st[:, 2 * j, 0] + st[:, 2 * j + 1, 0])
                    sq = sq + (st[:, 2 * j, 1] + st[:, 2 * j + 1, 1])
            halves.append((sm, sq))
        sm, sq = halves[0][0] + halves[1][0], halves[0][1] + halves[1][1]
        inv = f32(1.0) / f32(float(o.K))
        mean = sm * inv
        var = (sq * inv - mean * mean).clamp_min(0.0)
        rs = torch.rsqrt(var if defect == "no_eps" else var + f32(o.eps))
        nm = -mean * rs
        if defect == "act_before_bias":
            pre = act32(name, acc * rs[:, None] + o.fold_c[None, :] * nm[:, None]) + bias
            return {"out": pre.to(torch.bfloat16)}
        pre = acc * rs[:, None] + (o.fold_c[None, :] * nm[:, None] + bias)
        return {"out": act32(name, pre).to(torch.bfloat16)}
    if epi in (0, 1, 2, 6):
        v = act32(name, acc) + bias if defect == "act_before_bias" else act32(name, acc + bias)
        out = v.to(torch.bfloat16)
        if epi != 6:
            return {"out": out}
        return {"out": out, "stats": _stats32(v if defect == "stats_unrounded" else out.float(), defect)}
    v = acc + bias
    h = torch.zeros(o.M, o.N) if zero_h else o.h
    if epi == 3:
        return {"out": v.to(torch.bfloat16), "resid": h + v}
    a = torch.zeros(o.M, o.N)
    if with_addend:
        a = o.addend.float()
        if defect == "addend_ldr" and ldr is not None:
            buf = torch.full((o.M, ld_addend), float("nan"))
            buf[:, :o.N] = a
            flat = torch.cat([buf.reshape(-1), torch.full((o.M * max(ldr - ld_addend, 0) + o.N,), float("nan"))])
            a = flat[(torch.arange(o.M)[:, None] * ldr + torch.arange(o.N)[None, :])]
    s = f32(o.scale)
    r = h + s * (v + a) if defect == "scale_on_addend" else (h + v * s) + a
    if epi == 4:
        return {"resid": r}
    hb = r.to(torch.bfloat16)
    return {"resid": r, "hb": hb, "stats": _stats32(r if defect == "stats_unrounded" else hb.float(), defect)}
