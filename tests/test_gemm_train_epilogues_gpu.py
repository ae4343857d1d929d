"""GPU: the training-step GEMM epilogues and the patch-embedding epilogue in isolation (taps `ch_debug_gemm_train`,
`ch_debug_gemm_patch`), against fp64 on the same bf16-rounded operands, at ragged M, wide leading dimensions and the tails of the
activations -- where a fused epilogue goes wrong first.  u = 2^-8 (bf16), gamma_K = K 2^-24 / (1 - K 2^-24).

DACT (11 quick_gelu', 12 s * gelu'):  want = s (X W^T + bias) act'(aux);
    |got - want| <= (2u + u^2) |want| + gamma_K (|X||W|^T + |bias|) |s act'| + |s z| delta
    (two bf16 roundings: the staged acc + bias and the output; the fp32 accumulation; the derivative approximation).
ACT2 (13, 14):  the first output takes the bound of the LayerNorm-folded consumers (tests/test_gemm_gpu.py) and, on top of it, the
    derived bound of epilogue 8 (tests/gemm_ref.py: the exact function of the operands, the fp32 partials included); the second is checked
    against the activation of the kernel's OWN first output, in fp64: |hb - act(pre_got)| <= u |act| + delta_act.
PATCH (5):  patch rows of the fp32 residual within gamma_K |X||W|^T + 2^-24 |want| of X W^T + pos[1 + patch]; every other row untouched.

delta / delta_act: the absolute error of gemm_epilogue.h's formulas (dquick_gelu_f, dgelu_erf_f, quick_gelu_f, gelu_erf_f), evaluated
in fp32 on the CPU against the exact function in fp64 over every bf16 value the test can feed them (|x| <= 1e4 for aux, |x| <= 256 for
the pre-activations); `_deltas()` computes them once per run and prints them.  Measured: delta quick_gelu' 9.4e-7, gelu' 2.7e-7;
delta_act quick_gelu 6.3e-7, gelu 4.4e-7.

Which kernel takes which epilogue is listed in `_train_supported` / `_patch_supported`, not asked of the library: a narrowed
`*_supported` predicate fails here.
Every case prints its worst error / bound ratio (-s)."""
import pytest
import torch

from gemm_ref import SPECIAL, SPECIAL_COLS, Ops, _deltas, _dgelu, _dquick, _gelu, _quick, fold_operands, operands, out_ref
from kernel_launch import SENT16, sentinel as _sentinel, untouched as _untouched

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
U32 = 2.0 ** -24
EPI_PATCH, DACT_QUICK, DACT_GELU, ACT2_QUICK, ACT2_GELU = 5, 11, 12, 13, 14
MS = (1, 127, 129, 255, 257, 300)
SHAPES = ((128, 128), (384, 768), (768, 384), (256, 1280))      # (N, K)
VARIANTS = (0, 1, 2, 4, 7)               # dispatcher, 128x128 two-phase, 256x256 ping-pong (fine, coarse schedule), ring


def _experiments(lib):
    return bool(lib.ch_debug_experiments_built())


def _train_supported(lib, variant, N, K):
    """EXPECTED support of epilogues 11 .. 14: the dispatcher and the 128x128 kernel take every shape here; the 256x256 kernel needs
    N % 256 == 0 and K % 128 == 0 (its coarse schedule exists in an experiments build only); the ring carries forward epilogues only."""
    pp = {(128, 128): False, (384, 768): False, (768, 384): True, (256, 1280): True, (768, 768): True}[(N, K)]
    return {0: True, 1: True, 2: pp, 4: pp and _experiments(lib), 7: False}[variant]


def _patch_supported(lib, variant, N):
    """EXPECTED support of the patch epilogue at N = 128 / 384: not the 256x256 kernel (N % 256 != 0); the ring does carry it."""
    return {0: True, 1: True, 2: False, 4: False, 7: True}[variant]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from concepthash_amd import _lib
    return _lib.load()


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def _ratio(got, want, bound, what):
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    r = float(((got - want).abs() / bound).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: error exceeds the bound, worst ratio {r:.3f}"
    return r


def _operands(M, N, K, seed):
    return operands(M, N, K, seed, "cuda")


def _train(lib, variant, X, W, bias, M, epi, out, ldo, aux=None, scale=None, stats=None, fold_c=None, eps=1e-5, hb=None, ld_hb=0):
    from concepthash_amd import _lib
    N, K = W.shape
    rc = lib.ch_debug_gemm_train(variant, _lib.ptr(X), X.shape[0], _lib.ptr(W), _lib.ptr(bias), M, N, K, epi, _lib.ptr(out), ldo,
                                 _lib.ptr(aux), _lib.ptr(scale), _lib.ptr(stats), _lib.ptr(fold_c), eps, _lib.ptr(hb), ld_hb, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ---- DACT ------------------------------------------------------------------------------------------------------------------------
def _dact_case(M, N, K, ldo):
    g, Mp, X, W, bias = _operands(M, N, K, seed=17)
    a = 3.0 * torch.randn(M, N, generator=g, device="cuda")
    for col, val in zip(SPECIAL_COLS, SPECIAL):
        a[:, col] = val
    aux = torch.full((Mp, ldo), float("nan"), dtype=torch.bfloat16, device="cuda")      # NaN in the gap and past row M
    aux[:M, :N] = a.to(torch.bfloat16)
    Xd, Wd = X[:M].double(), W.double()
    z = Xd @ Wd.t() + bias.double()
    mag = Xd.abs() @ Wd.abs().t() + bias.double().abs()
    return X, W, bias, aux, z, mag


def _dact_check(lib, variant, M, N, K, ldo, case, epi, scale):
    X, W, bias, aux, z, mag = case
    what = f"dact epi {epi} variant {variant} M {M} N {N} K {K} ldo {ldo} scale {scale}"
    out = _sentinel(X.shape[0], ldo)
    sc = torch.tensor([scale], device="cuda") if scale is not None else None
    rc = _train(lib, variant, X, W, bias, M, epi, out, ldo, aux=aux, scale=sc)
    if not _train_supported(lib, variant, N, K):
        assert rc != 0 and lib.ch_last_error(), what + ": an unsupported combination must return a status"
        assert bool((out == SENT16).all()), what
        return
    assert rc == 0, (what, lib.ch_last_error())
    s = scale if (scale is not None and epi == DACT_GELU) else 1.0          # epilogue 11 ignores the scale
    d = (_dquick if epi == DACT_QUICK else _dgelu)(aux[:M, :N].double())
    want = s * z * d
    delta = _deltas()["dquick" if epi == DACT_QUICK else "dgelu"]
    bound = (2 * U + U * U) * want.abs() + gamma(K) * mag * (s * d).abs() + (s * z).abs() * delta
    _ratio(out.view(torch.bfloat16)[:M, :N], want, bound, what)
    assert _untouched(out, M, N), what + ": rows >= M or gap columns were written"


@pytest.mark.parametrize("N,K", SHAPES)
def test_derivative_epilogues(lib, N, K):
    for M in MS:
        for ldo in (N, N + 64):
            case = _dact_case(M, N, K, ldo)
            for variant in VARIANTS:
                _dact_check(lib, variant, M, N, K, ldo, case, DACT_QUICK, 0.37)      # the scale must be ignored
                _dact_check(lib, variant, M, N, K, ldo, case, DACT_GELU, None)
                _dact_check(lib, variant, M, N, K, ldo, case, DACT_GELU, 0.37)


def test_derivative_epilogue_refuses_aliased_aux(lib):
    """Training never runs the derivative epilogue in place; the tap refuses overlapping aux / out instead of racing."""
    M, N, K = 129, 128, 128
    X, W, bias, aux, _, _ = _dact_case(M, N, K, N)
    before = aux.clone()
    for epi in (DACT_QUICK, DACT_GELU):
        assert _train(lib, 1, X, W, bias, M, epi, aux, N, aux=aux) != 0 and lib.ch_last_error()
        assert _train(lib, 1, X, W, bias, M, epi, aux[64:], N, aux=aux) != 0
    assert torch.equal(aux.view(torch.int16), before.view(torch.int16))
    assert _train(lib, 1, X, W, bias, M, 10, _sentinel(X.shape[0], N), N, aux=aux) != 0      # not a training epilogue
    assert _train(lib, 3, X, W, bias, M, DACT_GELU, _sentinel(X.shape[0], N), N, aux=aux) != 0   # not a variant of this tap


# ---- ACT2 ------------------------------------------------------------------------------------------------------------------------
def _fold_case(M, N, K):
    """The LayerNorm-folded operands of tests/test_gemm_gpu.py::test_layernorm_folded_consumers"""
    return fold_operands(M, N, K, "cuda")


def _fold_first_output(X, Wf, d, c, stats, M):
    """(want, bound) of the first output by tests/gemm_ref.py: the exact function of these operands, the fp32 partials included"""
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    return out_ref(8, Ops(X[:M], Wf, d, stats=stats[:M], fold_c=c, eps=eps))


@pytest.mark.parametrize("N,K", SHAPES)
def test_two_output_epilogues(lib, N, K):
    for M in MS:
        X, Wf, d, c, stats, pre = _fold_case(M, N, K)
        want1, bound1 = _fold_first_output(X, Wf, d, c, stats, M)
        for ldo, ld_hb in ((N, N + 64), (N + 64, N + 128)):
            for variant in VARIANTS:
                for epi in (ACT2_QUICK, ACT2_GELU):
                    what = f"act2 epi {epi} variant {variant} M {M} N {N} K {K} ldo {ldo} ld_hb {ld_hb}"
                    out, hb = _sentinel(X.shape[0], ldo), _sentinel(X.shape[0], ld_hb)
                    rc = _train(lib, variant, X, Wf, d, M, epi, out, ldo, stats=stats, fold_c=c, hb=hb, ld_hb=ld_hb)
                    if not _train_supported(lib, variant, N, K):
                        assert rc != 0 and lib.ch_last_error(), what + ": an unsupported combination must return a status"
                        assert bool((out == SENT16).all()) and bool((hb == SENT16).all()), what
                        continue
                    assert rc == 0, (what, lib.ch_last_error())
                    got = out.view(torch.bfloat16)[:M, :N].float()
                    assert bool(torch.isfinite(got).all()), what
                    err = (got - pre.float()).abs()
                    print(f"{what}: first output max err {float(err.max()):.3e} rms {float(err.pow(2).mean().sqrt()):.3e}")
                    assert torch.allclose(got, pre.float(), atol=3e-2, rtol=2 ** -7), (what, float(err.max()))
                    assert float(err.pow(2).mean().sqrt()) < 6e-3, what
                    _ratio(got, want1, bound1, what + " first output")
                    quick = epi == ACT2_QUICK
                    act = (_quick if quick else _gelu)(got.double())
                    bound = U * act.abs() + _deltas()["quick" if quick else "gelu"]
                    _ratio(hb.view(torch.bfloat16)[:M, :N], act, bound, what + " second output")
                    assert _untouched(out, M, N) and _untouched(hb, M, N), what + ": rows >= M or gap columns were written"


# ---- the dispatcher's own 256x256 case ---------------------------------------------------------------------------------------------
def test_smallest_m_the_dispatcher_sends_to_the_256x256_kernel(lib):
    """ch_gemm_bf16 takes the 256x256 kernel from K >= 512 and ceil(M / 256) * (N / 256) >= 128 tiles: at N = 768 that is 43 row tiles,
    M = 42 * 256 + 1 = 10753 -- one row fewer stays on the 128x128 path (the dispatch counter shows both)."""
    N, K, M = 768, 768, 42 * 256 + 1
    count = lambda: [int(lib.ch_debug_gemm_dispatch_count(i)) for i in (0, 1)]
    case = _dact_case(M, N, K, N + 64)
    for epi, scale in ((DACT_QUICK, None), (DACT_GELU, 0.37)):
        c0 = count()
        _dact_check(lib, 0, M, N, K, N + 64, case, epi, scale)
        c1 = count()
        assert c1[1] - c0[1] == 1 and c1[0] == c0[0], "10753 rows did not reach the 256x256 kernel"
        _dact_check(lib, 0, M - 1, N, K, N + 64, (case[0], case[1], case[2], case[3], case[4][:M - 1], case[5][:M - 1]), epi, scale)
        c2 = count()
        assert c2[0] - c1[0] == 1 and c2[1] == c1[1], "10752 rows should stay on the 128x128 path"
    X, Wf, d, c, stats, pre = _fold_case(M, N, K)
    want1, bound1 = _fold_first_output(X, Wf, d, c, stats, M)
    for epi in (ACT2_QUICK, ACT2_GELU):
        out, hb = _sentinel(X.shape[0], N + 64), _sentinel(X.shape[0], N + 128)
        c0 = count()
        assert _train(lib, 0, X, Wf, d, M, epi, out, N + 64, stats=stats, fold_c=c, hb=hb, ld_hb=N + 128) == 0, lib.ch_last_error()
        c1 = count()
        assert c1[1] - c0[1] == 1 and c1[0] == c0[0]
        got = out.view(torch.bfloat16)[:M, :N].float()
        assert torch.allclose(got, pre.float(), atol=3e-2, rtol=2 ** -7)
        assert float((got - pre.float()).pow(2).mean().sqrt()) < 6e-3
        _ratio(got, want1, bound1, f"act2 epi {epi} dispatcher M {M} first output")
        quick = epi == ACT2_QUICK
        act = (_quick if quick else _gelu)(got.double())
        _ratio(hb.view(torch.bfloat16)[:M, :N], act, U * act.abs() + _deltas()["quick" if quick else "gelu"], f"act2 epi {epi} dispatcher M {M}")
        assert _untouched(out, M, N) and _untouched(hb, M, N)


# ---- PATCH -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [640, 768])
def test_patch_epilogue(lib, N, K):
    from concepthash_amd import _lib
    sent = -12345.5
    for npatch in (4, 9, 49):
        for Q in (0, 4):
            for nimg in (1, 3):
                M, ntok = nimg * npatch, 1 + npatch + Q
                g, Mp, X, W, _ = _operands(M, N, K, seed=23)
                pos = torch.randn(1 + npatch, N, generator=g, device="cuda")
                Xd, Wd = X[:M].double(), W.double()
                want = Xd @ Wd.t() + pos[1:].double().repeat(nimg, 1)
                bound = gamma(K) * (Xd.abs() @ Wd.abs().t()) + U32 * want.abs()
                is_patch = torch.zeros(nimg * ntok + 5, dtype=torch.bool, device="cuda")
                for b in range(nimg):
                    is_patch[b * ntok + 1:b * ntok + 1 + npatch] = True
                for variant in VARIANTS:
                    what = f"patch variant {variant} N {N} K {K} patches {npatch} Q {Q} images {nimg}"
                    resid = torch.full((nimg * ntok + 5, N), sent, device="cuda")
                    rc = lib.ch_debug_gemm_patch(variant, _lib.ptr(X), Mp, _lib.ptr(W), M, N, K, _lib.ptr(resid), N, _lib.ptr(pos), ntok, npatch,
                                                 _lib.stream_ptr())
                    torch.cuda.synchronize()
                    if not _patch_supported(lib, variant, N):
                        assert rc != 0 and lib.ch_last_error(), what + ": an unsupported combination must return a status"
                        assert bool((resid == sent).all()), what
                        continue
                    assert rc == 0, (what, lib.ch_last_error())
                    _ratio(resid[is_patch], want, bound, what)
                    assert bool((resid[~is_patch] == sent).all()), what + ": a CLS / concept row or a row past the last image was written"
