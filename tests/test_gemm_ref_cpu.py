"""CPU: the bounds of tests/gemm_ref.py have teeth.  The clean emulation of every forward epilogue stays inside every bound at every
shape tests/test_gemm_fwd_epilogues_gpu.py runs, and each defect of `gemm_ref.DEFECTS` leaves a bound (or breaks a bit equality) at one
of them.  Prints the clean emulation's worst error / bound ratio per epilogue family (-s)."""
import pytest
import torch

import gemm_ref as gr

MS = (1, 127, 129, 255, 257, 300)
SHAPES = ((128, 64), (128, 96), (384, 768), (768, 384), (256, 1280))      # (N, K), general
FOLD_SHAPES = tuple((N, K) for K in (128, 640, 1152, 1280) for N in (256, 384))
WIDE = dict(ldr=32, ld_addend=96)                                         # what the wide launches add to N
SPLITK = {256: 2, 768: 6, 1280: 5, 3072: 8}                               # K -> slices (N = 256, 256 compute units)
_worst = {}


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(kind, M, N, K):
        key = (kind, M, N, K)
        if key not in made:
            made[key] = (gr.fold_case if kind == "fold" else gr.fwd_case)(M, N, K, device="cpu")
        return made[key]
    return get


def _run(epi, o, defect=None, **kw):
    emu = {k: kw[k] for k in ("split", "ldr", "ld_addend") if k in kw}
    chk = {k: kw[k] for k in ("with_addend", "zero_h") if k in kw}
    return gr.checks(epi, o, gr.emulate(epi, o, defect=defect, **emu, **chk), **chk)


def _clean(epi, o, **kw):
    res = _run(epi, o, **kw)
    assert not gr.failed(res), (epi, o.M, o.N, o.K, kw, gr.failed(res))
    for r in res:
        if r[0] == "bound":
            ratio = float(((r[3].double() - r[4]).abs() / r[5]).max())
            _worst[r[1]] = max(_worst.get(r[1], 0.0), ratio)


def test_lipschitz_constants_and_deltas():
    x = torch.linspace(-40.0, 40.0, 800001, dtype=torch.float64)
    for name, d in (("quick", gr._dquick), ("gelu", gr._dgelu)):
        lo, hi = float(d(x).min()), float(d(x).max())
        print(f"{name}': [{lo:.4f}, {hi:.4f}]")
        assert max(-lo, hi) <= gr.LIPSCHITZ[name] < max(-lo, hi) + 0.01
    dl = gr._deltas()
    assert 0.0 < dl["quick"] < 2e-6 and 0.0 < dl["gelu"] < 2e-6
    # past the measured range both formulas return x, or a zero, exactly: every finite bf16 |x| > 256
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16).float()
    v = v[torch.isfinite(v) & (v.abs() > 256)]
    for name in ("quick", "gelu"):
        got = gr.act32(name, v)
        assert bool((got == torch.where(v > 0, v, torch.zeros_like(v))).all()), name
        assert bool(((got.double() - gr.act64(name, v.double())).abs() <= gr.TINY).all()), name


@pytest.mark.parametrize("N,K", SHAPES)
def test_clean_emulation_general(cases, N, K):
    for M in MS:
        o = cases("fwd", M, N, K)
        for epi in (0, 1, 2, 6):
            _clean(epi, o)
        _clean(3, o)
        _clean(3, o, zero_h=True)
        for epi in (4, 7):
            _clean(epi, o, with_addend=False)
            _clean(epi, o, ldr=N + WIDE["ldr"], ld_addend=N + WIDE["ld_addend"])
    print("WORST " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_worst.items())))


@pytest.mark.parametrize("N,K", FOLD_SHAPES)
def test_clean_emulation_fold(cases, N, K):
    for M in MS:
        o = cases("fold", M, N, K)
        for epi in gr.FOLD:
            _clean(epi, o)
    print("WORST " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_worst.items())))


@pytest.mark.parametrize("K", sorted(SPLITK))
def test_clean_emulation_split_k(cases, K):
    for M in (1, 257, 300):
        o = cases("fwd", M, 256, K)
        for epi in (0, 1, 2, 3, 6):
            _clean(epi, o, split=SPLITK[K])
        for epi in (4, 7):
            _clean(epi, o, split=SPLITK[K])
        if K <= 1280:
            f = cases("fold", M, 256, K)
            for epi in gr.FOLD:
                _clean(epi, f, split=SPLITK[K])
    print("WORST " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_worst.items())))


def _candidates(defect, cases):
    """(epi, operands, keyword arguments) in which `defect` is active, smallest first"""
    wide = lambda N: dict(ldr=N + WIDE["ldr"], ld_addend=N + WIDE["ld_addend"])
    for M in (129, 300):
        if defect in ("drop_last_ktile", "bias_col_plus_1"):
            for N, K in SHAPES:
                for epi in (0, 1, 2, 3, 4, 6, 7):
                    yield epi, cases("fwd", M, N, K), {}
            for N, K in FOLD_SHAPES[:2]:
                for epi in gr.FOLD:
                    yield epi, cases("fold", M, N, K), {}
        elif defect == "no_eps":
            for N, K in FOLD_SHAPES:
                for epi in gr.FOLD:
                    yield epi, cases("fold", M, N, K), {}
        elif defect in ("stats_next_slice", "stats_unrounded"):
            for N, K in SHAPES:
                for epi in (6, 7):
                    yield epi, cases("fwd", M, N, K), {}
        elif defect in ("scale_on_addend", "addend_ldr"):
            for N, K in SHAPES:
                for epi in (4, 7):
                    yield epi, cases("fwd", M, N, K), wide(N)
        elif defect == "splitk_drop_slice":
            for K in sorted(SPLITK):
                for epi in (0, 4):
                    yield epi, cases("fwd", M, 256, K), dict(split=SPLITK[K])
        elif defect == "act_before_bias":
            for N, K in SHAPES:
                for epi in (1, 2):
                    yield epi, cases("fwd", M, N, K), {}
            for N, K in FOLD_SHAPES[:2]:
                for epi in (9, 10):
                    yield epi, cases("fold", M, N, K), {}


@pytest.mark.parametrize("defect", gr.DEFECTS)
def test_every_defect_leaves_a_bound(cases, defect):
    """every epilogue the defect applies to must catch it at the smallest shape it runs at"""
    caught = {}
    for epi, o, kw in _candidates(defect, cases):
        if caught.get(epi):
            continue
        bad = gr.failed(_run(epi, o, defect=defect, **kw))
        caught[epi] = caught.get(epi, False) or bool(bad)
        if bad:
            print(f"{defect}: epilogue {epi} M {o.M} N {o.N} K {o.K} fails {bad}")
    assert caught and all(caught.values()), (defect, caught)


def test_addend_defect_needs_distinct_leading_dimensions(cases):
    """with ldr == ld_addend the mix-up cannot show: why the GPU test runs every leading dimension wide and pairwise different"""
    o = cases("fwd", 129, 128, 96)
    assert not gr.failed(_run(4, o, defect="addend_ldr", ldr=128, ld_addend=128))
    assert gr.failed(_run(4, o, defect="addend_ldr", ldr=128 + 32, ld_addend=128 + 96))
