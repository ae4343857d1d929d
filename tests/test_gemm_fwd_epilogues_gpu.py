"""GPU: the ten forward epilogues of the bf16 GEMM family (0 .. 4, 6 .. 10), one launch at a time through `ch_debug_gemm_fwd`, against the
fp64 references and derived bounds of tests/gemm_ref.py (its docstring derives every term; tests/test_gemm_ref_cpu.py shows on the CPU
that each bound catches the defects it is there for), in the launch discipline of tests/kernel_launch.py: every output starts as a
sentinel between guard blocks, with sentinel rows behind row M and sentinel gap columns behind column N; every input is followed by NaN,
the rows of X between M and the next multiple of 256 and the gaps of the addend are NaN too; a second identical launch must give the
same bytes.

Which kernel takes which (N, K, epilogue) is written down in `_supported`, not asked of the library; an unsupported combination must
return a status, set ch_last_error() and leave every output as it was.  Variant 0 is the dispatcher's rule; 1 (128x128 two-phase),
2 / 4 (256x256 ping-pong, fine / coarse schedule; 4 in an experiments build only) and 7 (128x128 ring) are forced THROUGH the
dispatcher.  Every leading dimension runs tight and wide (ldo = N + 64, ldr = N + 32, ld_addend = N + 96, ld_hb = N + 128: pairwise
different, so that a mix-up cannot cancel).

Exact grid: with X the 256 x 256 bf16 identity, bias 0 and W holding all 65,536 bf16 bit patterns (inf, NaN and subnormals replaced by
zero) the pre-activation of output (m, n) is W[n][m] exactly -- every other product is an exact zero -- so every finite normal bf16
value goes through each fused activation once, +-88, +-1e4 and +-3e38 included.  Subnormal inputs are left out because nobody has
measured whether the MFMA keeps them.

Split-K: `splitk = 1` on variant 2 splits EVERY tile of a problem with fewer tiles than compute units.  The slice count cannot be read
back from a launch; `_split_s` restates ch_pp_choose_split and is asserted to give S = 2, 6, 5, 8 for K = 256, 768, 1280, 3072 on the
256 compute units of an MI355X, so a test run on another device says so instead of silently testing another split.

Measured on an MI355X, product build and experiments build (variant 4 included) alike -- worst error / bound per group, printed by
every test (-s):
    plain 0.993 | fold 0.990 | residual 0.894 | stats 0.052 (order-free gamma_64 / gamma_65) | stats tree 0.486 (gamma_7)
    exact grid: quick_gelu 0.996, gelu 0.968;  delta_act quick_gelu 6.32e-7, gelu 4.44e-7 (delta of the derivatives 9.39e-7, 2.68e-7)
The bf16 groups sit at u / (1 + u) = 0.996 of u |want|: a rounding near a tie just above a power of two attains the rounding term, so
their ratio says that nothing ELSE pushed an element out, not how much room the other terms have; the residual group has no bf16
rounding and shows the fp32 terms alone.  The statistics' bound of record is the order-free one and is slack by the ratio of
63 additions to the trees' 7; the tree bound next to it is the one with teeth.
Sensitivity, one scratch build with three in-bounds defects (addend indexed with ldr; ln_eps left out; slice 0 left out of the split-K
sum), this file run once, every failure an assertion: 19 of 30 tests fail -- the 5 general and 8 fold cases, the 4 split-K cases
(ratio 110 .. 2582 at epilogue 0), the non-temporal and the tile-order test (epilogues 4 / 7, wide) -- and the exact grid, the
refusals and the dispatcher-rule test (bytes only) pass.
"""
import pytest
import torch

import gemm_ref as gr
from kernel_launch import SENT32, Out, inp, report, twice, within

pytestmark = pytest.mark.gpu

MS = (1, 127, 129, 255, 257, 300)
SHAPES = ((128, 64), (128, 96), (384, 768), (768, 384), (256, 1280))      # (N, K), general
FOLD_SHAPES = tuple((N, K) for K in (128, 640, 1152, 1280) for N in (256, 384))
VARIANTS = (0, 1, 2, 4, 7)
PAST = 3                                  # sentinel rows behind row M of every output
SPLIT_S = {256: 2, 768: 6, 1280: 5, 3072: 8}
GROUPS = ("plain", "residual", "stats", "stats tree", "fold")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from concepthash_amd import _lib
    return _lib.load()


def _experiments(lib):
    return bool(lib.ch_debug_experiments_built())


def _supported(lib, variant, N, K, epi):
    """EXPECTED support.  Two-phase (1): K % 64 == 0.  Ping-pong (2; 4 = its coarse schedule, experiments build only): N % 256 == 0 and
    K % 128 == 0.  Ring (7): K % 32 == 0 and K >= 96.  The rule (0) at these row counts: the ring where it is supported, otherwise the
    two-phase kernel.  N % 128 == 0 everywhere here; the fold epilogues need K % 128 == 0 and K <= 1280 on top."""
    v1, pp, ring = K % 64 == 0, N % 256 == 0 and K % 128 == 0, K % 32 == 0 and K >= 96
    ok = {0: v1 or ring, 1: v1, 2: pp, 4: pp and _experiments(lib), 7: ring}[variant]
    return ok and (epi not in gr.FOLD or (K % 128 == 0 and K <= 1280))


def _lds(N, wide):
    return dict(ldo=N + 64, ldr=N + 32, lda=N + 96, ldh=N + 128) if wide else dict(ldo=N, ldr=N, lda=N, ldh=N)


class Dev:
    """the device-side inputs of one `gr.Ops`, each followed by NaN; X padded to a multiple of 256 rows of NaN"""

    def __init__(self, o):
        self.o, dev = o, "cuda"
        self.Mp = (o.M + 255) // 256 * 256
        Xp = torch.full((self.Mp, o.K), float("nan"), dtype=torch.bfloat16)
        Xp[:o.M] = o.X.cpu()
        self.X, self.W, self.bias = inp(dev, Xp), inp(dev, o.W.cpu()), inp(dev, o.bias.cpu())
        self.scale = inp(dev, torch.tensor([o.scale], dtype=torch.float32)) if o.scale is not None else None
        self.stats = inp(dev, o.stats.cpu()) if o.stats is not None else None
        self.fold_c = inp(dev, o.fold_c.cpu()) if o.fold_c is not None else None
        self._addend, self._h = {}, {}

    def addend(self, ld):
        if ld not in self._addend:
            a = torch.full((self.o.M, ld), float("nan"), dtype=torch.bfloat16)
            a[:, :self.o.N] = self.o.addend.cpu()
            self._addend[ld] = inp("cuda", a)
        return self._addend[ld]

    def resid(self, ld, zero_h):
        """an in / out residual [M + PAST, ld]: h in the valid part, the sentinel in the gap and behind row M"""
        key = (ld, zero_h)
        if key not in self._h:
            r = torch.full((self.o.M + PAST, ld), SENT32, dtype=torch.int32).view(torch.float32)
            r[:self.o.M, :self.o.N] = 0.0 if zero_h else self.o.h.cpu()
            self._h[key] = r
        return Out("cuda", self._h[key].shape, torch.float32, init=self._h[key])


def _run(lib, dv, epi, variant, wide=False, with_addend=True, zero_h=False, nt_resid=0, nt_out=0, group_n=0, rev=0, splitk=0):
    """one launch on fresh outputs -> (status, {name: Out})"""
    from concepthash_amd import _lib
    o, ld = dv.o, _lds(dv.o.N, wide)
    M, N, K = o.M, o.N, o.K
    outs = {}
    if epi not in (4, 7):
        outs["out"] = Out("cuda", (M + PAST, ld["ldo"]), torch.bfloat16)
    if epi in (3, 4, 7):
        outs["resid"] = dv.resid(ld["ldr"], zero_h)
    if epi == 7:
        outs["hb"] = Out("cuda", (M + PAST, ld["ldh"]), torch.bfloat16)
    if epi in (6, 7):
        outs["stats"] = Out("cuda", (M + PAST, N // 64, 2), torch.float32)
    ptr = lambda name: outs[name].ptr if name in outs else None
    addend = dv.addend(ld["lda"]) if (epi in (4, 7) and with_addend) else None
    rc = lib.ch_debug_gemm_fwd(variant, _lib.ptr(dv.X), dv.Mp, _lib.ptr(dv.W), _lib.ptr(dv.bias), M, N, K, epi, ptr("out"), ld["ldo"],
                               ptr("resid"), ld["ldr"], _lib.ptr(dv.scale) if epi in (4, 7) else None, _lib.ptr(addend), ld["lda"],
                               _lib.ptr(dv.stats) if epi in gr.FOLD else None, _lib.ptr(dv.fold_c) if epi in gr.FOLD else None,
                               o.eps if epi in gr.FOLD else 0.0, ptr("stats"), ptr("hb"), ld["ldh"], nt_resid, nt_out, group_n, rev, splitk,
                               _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, outs


def _valid(outs, M, N):
    """{name: payload of the valid rows and columns}, after checking that everything else is still what it was"""
    got = {}
    for name, x in outs.items():
        full = x.get()
        mask = torch.ones(x.shape, dtype=torch.bool)
        if name == "stats":
            mask[:M] = False
            got[name] = full[:M]
        else:
            mask[:M, :N] = False
            got[name] = full[:M, :N]
        assert x.untouched(mask), f"{name}: a row >= M or a gap column was written"
    return got


def _bytes(outs):
    return {k: v.raw().clone() for k, v in outs.items()}


def _refused(lib, dv, epi, variant, what, **kw):
    rc, outs = _run(lib, dv, epi, variant, **kw)
    assert rc != 0 and lib.ch_last_error(), what + ": an unsupported combination must return a status"
    for name, x in outs.items():
        if name == "resid":
            assert torch.equal(x.raw(), dv.resid(x.shape[1], kw.get("zero_h", False)).raw()), what + ": resid was written"
        else:
            assert x.untouched(torch.ones(x.shape, dtype=torch.bool)), what + f": {name} was written"


def _check(lib, dv, epi, variant, times=2, **kw):
    """`times` identical launches with equal bytes, every check of gemm_ref.checks, nothing written outside the valid part"""
    o = dv.o
    what = f"epi {epi} variant {variant} M {o.M} N {o.N} K {o.K} {kw}"
    if not _supported(lib, variant, o.N, o.K, epi):
        _refused(lib, dv, epi, variant, what, **kw)
        return None
    names = []

    def launch():
        rc, outs = _run(lib, dv, epi, variant, **kw)
        assert rc == 0, (what, lib.ch_last_error())
        names[:] = list(outs)
        return list(outs.values())
    first = twice(launch)
    for _ in range(times - 2):
        for a, b in zip(first, launch()):
            assert torch.equal(a.raw(), b.raw()), what + ": a further identical launch gave other bytes"
    outs = dict(zip(names, first))
    got = _valid(outs, o.M, o.N)
    ck = {k: kw[k] for k in ("with_addend", "zero_h") if k in kw}
    for r in gr.checks(epi, o, got, **ck):
        if r[0] == "equal":
            assert torch.equal(r[3], r[4]), f"{what}: {r[2]}"
        else:
            within(r[1], r[3], r[4], r[5], f"{what} {r[2]}")
    return outs


def _epilogue_runs(epi_set):
    runs = []
    for epi in epi_set:
        if epi == 3:
            runs += [(3, {}), (3, dict(zero_h=True))]
        elif epi == 4:
            runs += [(4, dict(with_addend=False)), (4, {})]
        else:
            runs.append((epi, {}))
    return runs


# ---- 1. every epilogue within its bound ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_plain_residual_and_statistics_epilogues(lib, N, K):
    for M in MS:
        dv = Dev(gr.fwd_case(M, N, K))
        for wide in (False, True):
            for variant in VARIANTS:
                for epi, kw in _epilogue_runs((0, 1, 2, 3, 4, 6, 7)):
                    _check(lib, dv, epi, variant, wide=wide, **kw)
    report("plain", "residual", "stats", "stats tree")


@pytest.mark.parametrize("N,K", FOLD_SHAPES)
def test_fold_consumers(lib, N, K):
    for M in MS:
        dv = Dev(gr.fold_case(M, N, K))
        for wide in (False, True):
            for variant in VARIANTS:
                for epi in gr.FOLD:
                    _check(lib, dv, epi, variant, wide=wide)
    report("fold")


def test_the_tap_refuses_what_the_kernels_cannot_take(lib):
    """argument checks of ch_debug_gemm_fwd: leading dimensions below N or off the access width, aliased outputs, missing operands, an
    epilogue or a variant that is not the tap's, a split on a kernel that has none -- a status, and nothing written"""
    from concepthash_amd import _lib
    M, N, K = 129, 256, 128
    dv, fv = Dev(gr.fwd_case(M, N, K)), Dev(gr.fold_case(M, N, K))
    out, hb = Out("cuda", (M, N + 64), torch.bfloat16), Out("cuda", (M, N + 64), torch.bfloat16)
    resid, stats = Out("cuda", (M, N + 64), torch.float32), Out("cuda", (M, N // 64, 2), torch.float32)
    scale, addend = dv.scale, dv.addend(N + 96)

    def call(epi, variant=1, d=dv, X=True, bias=True, out=out, ldo=N, resid=resid, ldr=N, scale=scale, addend=None, lda=N, stats_in=None,
             fold_c=None, eps=1e-5, stats=stats, hb=hb, ldh=N, splitk=0, nt=0):
        p = lambda x: None if x is None else (x.ptr if isinstance(x, Out) else _lib.ptr(x))
        rc = lib.ch_debug_gemm_fwd(variant, _lib.ptr(d.X) if X else None, d.Mp, _lib.ptr(d.W), _lib.ptr(d.bias) if bias else None, M, N, K,
                                   epi, p(out), ldo, p(resid), ldr, p(scale), p(addend), lda, p(stats_in), p(fold_c), eps, p(stats), p(hb), ldh,
                                   nt, 0, 0, 0, splitk, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc != 0 and bool(lib.ch_last_error())

    assert call(0, X=False) and call(0, bias=False) and call(0, out=None)
    assert call(5) and call(11) and call(-1) and call(0, variant=3) and call(0, variant=8)
    assert call(0, ldo=N - 8) and call(0, ldo=N + 4) and call(3, ldo=N + 2) and call(3, ldr=N + 2) and call(3, resid=None)
    assert call(4, scale=None) and call(4, addend=addend, lda=N + 2) and call(4, addend=addend, lda=N - 4) and call(4, resid=None)
    assert call(6, stats=None) and call(7, stats=None) and call(7, hb=None) and call(7, ldh=N + 2) and call(7, ldh=N - 4)
    assert call(7, hb=resid) and call(3, out=resid)
    assert call(8, d=fv) and call(8, d=fv, stats_in=fv.stats) and call(8, d=fv, stats_in=fv.stats, fold_c=fv.fold_c, eps=0.0)
    assert call(0, splitk=1) and call(0, variant=7, splitk=1) and call(4, nt=2)
    for x in (out, hb, resid, stats):
        assert x.untouched(torch.ones(x.shape, dtype=torch.bool))
    assert not call(8, d=fv, stats_in=fv.stats, fold_c=fv.fold_c)             # and the well-formed call goes through
    assert not out.untouched(torch.ones(out.shape, dtype=torch.bool))


# ---- 2. exact grid ---------------------------------------------------------------------------------------------------------------------
def _grid_case():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    w = bits.view(torch.bfloat16).clone()
    f = w.float()
    w[~torch.isfinite(f) | ((f != 0) & (f.abs() < 2.0 ** -126))] = 0.0       # inf, NaN, subnormals
    X = torch.eye(256, dtype=torch.bfloat16)
    return gr.Ops(X, w.view(256, 256), torch.zeros(256), h=torch.zeros(256, 256))


@pytest.mark.parametrize("variant", [1, 2, 7])
def test_every_normal_bf16_value_through_every_fused_activation(lib, variant):
    o = _grid_case()
    dv = Dev(o)
    x = o.W.t().contiguous()                                                  # the pre-activation of (m, n) is W[n][m]
    assert int((x.float().abs() > 3.3e38).sum()) >= 2 and int((x.float().abs() == 88.0).sum()) == 2

    def one(epi, **kw):
        names = []

        def launch():
            rc, outs = _run(lib, dv, epi, variant, **kw)
            assert rc == 0, (epi, variant, lib.ch_last_error())
            names[:] = list(outs)
            return list(outs.values())
        return _valid(dict(zip(names, twice(launch))), 256, 256)
    got = one(0)["out"]
    assert torch.equal(got.float(), x.float()), "EPI_BIAS of the identity did not return W^T value for value"
    got = one(3, zero_h=True)
    assert torch.equal(got["resid"], x.float()) and torch.equal(got["out"].float(), x.float())
    for epi, name in ((1, "quick"), (2, "gelu")):
        want, bound = gr.act_bound(name, x.double())
        within(f"grid {name}", one(epi)["out"], want, bound, f"exact grid epi {epi} variant {variant}")
    report("grid quick", "grid gelu")


# ---- 3. split-K with every tile split ----------------------------------------------------------------------------------------------------
def _split_s(tiles, K, ncu):
    """ch_pp_choose_split (gemm_pp.hip) restated: the slices of each tile of the last, partial round"""
    R, J, S = tiles % ncu, K // 128, 1
    if R == 0:
        return 1
    for c in range(2, 9):
        if J % c == 0 and R * c <= ncu and R * c <= 256:
            S = c
    return S


@pytest.mark.parametrize("K", sorted(SPLIT_S))
def test_split_k_with_every_tile_split(lib, K):
    N = 256
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for M in (1, 257, 300):
        tiles = (M + 255) // 256 * (N // 256)
        assert tiles < ncu and _split_s(tiles, K, ncu) == SPLIT_S[K], (tiles, ncu, _split_s(tiles, K, ncu))
        dv = Dev(gr.fwd_case(M, N, K))
        for epi, kw in _epilogue_runs((0, 1, 2, 3, 4, 6, 7)):
            _check(lib, dv, epi, 2, times=3, splitk=1, wide=True, **kw)
        if K <= 1280:
            fv = Dev(gr.fold_case(M, N, K))
            for epi in gr.FOLD:
                _check(lib, fv, epi, 2, times=3, splitk=1, wide=True)
    report(*GROUPS)


# ---- 4. non-temporal instances ---------------------------------------------------------------------------------------------------------
def test_non_temporal_instances_give_the_same_bytes_and_are_counted(lib):
    M, N, K = 300, 768, 768
    dv, fv = Dev(gr.fwd_case(M, N, K)), Dev(gr.fold_case(M, N, K))
    count = lambda which: int(lib.ch_debug_gemm_dispatch_count(which))
    for which, variant, opt, cases in ((2, 1, "nt_resid", ((4, dv), (7, dv))), (3, 2, "nt_out", ((0, dv), (8, fv), (9, fv), (10, fv)))):
        for epi, d in cases:
            what = f"epi {epi} variant {variant} {opt}"
            c0 = count(which)
            plain = _check(lib, d, epi, variant, wide=True, **{opt: -1})
            assert count(which) == c0, what + ": the default-policy instance was counted as non-temporal"
            forced = _check(lib, d, epi, variant, wide=True, **{opt: 1})
            assert count(which) == c0 + 2, what + ": two forced launches must count two non-temporal launches"
            for k in plain:
                assert torch.equal(plain[k].raw(), forced[k].raw()), f"{what}: {k} differs from the default-policy instance"
    report(*GROUPS)


# ---- 5. tile order -----------------------------------------------------------------------------------------------------------------------
def test_tile_order_options_do_not_change_a_byte(lib):
    M, N, K = 700, 768, 768
    dv = Dev(gr.fwd_case(M, N, K))
    for variant in (1, 2, 4, 7):
        if variant == 4 and not _experiments(lib):
            continue
        tiles_n = N // (256 if variant in (2, 4) else 128)
        options = [dict(rev=1)] + [dict(group_n=g) for g in (1, 2, tiles_n)] + [dict(rev=1, group_n=2)]
        if variant in (1, 7):                                                 # six n-tiles: a group of four and a partial group of two
            options += [dict(group_n=4)]
        for epi in (0, 7):
            base = _check(lib, dv, epi, variant, wide=True)                   # sentinel payloads: no tile was skipped
            for opt in options:
                other = _check(lib, dv, epi, variant, wide=True, **opt)
                for k in base:
                    assert torch.equal(base[k].raw(), other[k].raw()), f"epi {epi} variant {variant} {opt}: {k} differs from the default order"


# ---- 6. the dispatcher's rule at these sizes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES + ((256, 640), (384, 1152)))
def test_dispatcher_rule_at_small_row_counts(lib, N, K):
    """up to 8,192 rows (and far below 128 tiles of 256 x 256) variant 0 is the ring where ch_gemm_r4_supported holds, otherwise the
    two-phase kernel; either way it is counted as a 128x128 launch and gives the forced variant's bytes"""
    count = lambda: [int(lib.ch_debug_gemm_dispatch_count(i)) for i in (0, 1)]
    expect = 7 if (K % 32 == 0 and K >= 96) else 1
    fold = (N, K) not in SHAPES
    for M in (129, 300):
        dv = Dev(gr.fold_case(M, N, K) if fold else gr.fwd_case(M, N, K))
        for epi in (gr.FOLD if fold else (0, 1, 2, 3, 4, 6, 7)):
            c0 = count()
            rc, ruled = _run(lib, dv, epi, 0, wide=True)
            c1 = count()
            assert rc == 0 and c1[0] == c0[0] + 1 and c1[1] == c0[1], (epi, M, N, K, lib.ch_last_error())
            rc, forced = _run(lib, dv, epi, expect, wide=True)
            assert rc == 0, lib.ch_last_error()
            for k in ruled:
                assert torch.equal(ruled[k].raw(), forced[k].raw()), f"epi {epi} M {M} N {N} K {K}: the rule did not run variant {expect}"
