"""CPU: the fp64 restatements and derived bounds of tests/train_kernels_ref.py are (a) sound -- an fp32 emulation of every operation in
ANOTHER summation order stays inside its bound on every input of tests/test_train_rowkernels_gpu.py, (b) equal to fp64 autograd where a
closed form is restated, and (c) sharp -- every deliberate defect breaches the bound somewhere, and every single case of the
operations that HAVE a bound catches at least one defect (a case whose bound no defect can breach would test nothing).  The transposes
and row moves are bit-exact, so there is no bound to be too wide: an independent emulation must equal the restatement bit for bit, and
each of its defects must differ from it in every case where the defect exists (a 1 x 1 transpose has none).  The worst error / bound
ratios are printed (-s)."""
import torch

import train_kernels_ref as tr


class Tally:
    """per operation: the worst clean ratio, which defects were caught at all, and that every case caught one"""

    def __init__(self, name, defects):
        self.name, self.defects, self.worst, self.caught = name, defects, 0.0, set()

    def clean(self, got, ref, bound, what):
        self.worst = max(self.worst, tr.assert_within(got, ref, bound, f"{self.name} {what}", quiet=True))

    def case(self, what, hits):
        """hits: {defect: breached?} of one case"""
        assert any(hits.values()), f"{self.name} {what}: no defect breaches the bound -- this case tests nothing"
        self.caught |= {d for d, h in hits.items() if h}

    def done(self):
        print(f"WORST {self.name}: {self.worst:.3f}")
        assert self.caught == set(self.defects), f"{self.name}: never caught {sorted(set(self.defects) - self.caught)}"
        assert self.worst <= 1.0


def _row_cases():
    return [(rows, D, fam) for D in tr.ROW_D for rows in tr.ROW_ROWS for fam in tr.ROW_FAMILIES]


def test_half_ulp_is_the_rounding_error_of_bf16():
    """the bf16 term: exact at a tie just above a power of two (where a flat 2^-9 relative would refuse the correct rounding), never exceeded"""
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.99, 200.4, 3e-5], dtype=torch.float32)
    err = (x.to(torch.bfloat16).double() - x.double()).abs()
    hu = tr.half_ulp_bf16(x.double().abs())
    assert bool((err <= hu).all()) and float(err[0]) == float(hu[0]) == 2.0 ** -8 and float(err[0]) > 2.0 ** -9 * float(x[0])
    v = torch.randn(100000, generator=tr.gen("half_ulp")) * torch.exp2(torch.randint(-20, 20, (100000,), generator=tr.gen("e")).float())
    err = (v.to(torch.bfloat16).double() - v.double()).abs()
    hu = tr.half_ulp_bf16(v.double().abs())
    assert bool((err <= hu).all()) and bool((hu <= 2.0 ** -8 * v.double().abs()).all()) and bool((hu > 2.0 ** -9 * v.double().abs()).all())


def test_hb_stats():
    t = Tally("hb_stats", tr.HB_STATS_DEFECTS)
    for rows, D, fam in _row_cases():
        H = tr.row_family(fam, rows, D)
        hb, ref, bound = tr.hb_stats_ref(H)
        ehb, est = tr.hb_stats_emul(H)
        assert tr.bits_equal(hb, ehb)
        t.clean(est, ref, bound, f"{fam} {rows}x{D}")
        t.case(f"{fam} {rows}x{D}", {d: tr.breaches(tr.hb_stats_emul(H, d)[1], ref, bound) for d in tr.HB_STATS_DEFECTS})
    t.done()


def test_normalize_and_the_statistics_path():
    t = Tally("normalize", tr.NORMALIZE_DEFECTS)
    worst_cancel = 0.0
    for rows, D, fam in _row_cases():
        x = tr.row_family(fam, rows, D).to(torch.bfloat16)
        stats = tr.hb_stats_emul(x.float())[1]
        ref, bound, (R, e_r, cancel) = tr.normalize_ref(x, stats)
        assert bool(torch.isfinite(e_r).all()), (fam, rows, D)
        t.clean(tr.normalize_emul(x, stats), ref, bound, f"{fam} {rows}x{D}")
        t.case(f"{fam} {rows}x{D}", {d: tr.breaches(tr.normalize_emul(x, stats, defect=d), ref, bound) for d in tr.NORMALIZE_DEFECTS})
        # rstd itself: the emulation's value against the exact one, inside e_r
        _, rstd = tr._mean_rstd_f32(stats, D, tr.LN_EPS)
        rel = ((rstd.double() - R).abs() / R)
        assert bool((rel <= e_r / R).all())
        if fam == "offset":
            worst_cancel = max(worst_cancel, float(cancel.max()))
            print(f"offset rows {rows}x{D}: cancellation factor {float(cancel.max()):.3g}, rstd relative error {float(rel.max()):.2e}"
                  f" (bound {float((e_r / R).max()):.2e})")
            # the bound must carry the cancellation: u32 * factor is its scale, and it must stay meaningful (well below 1)
            assert float((e_r / R).max()) > 0.5 * tr.U32 * float(cancel.max()) and float((e_r / R).max()) < 0.05
        elif fam == "benign":
            assert float((e_r / R).max()) < 1e-5
    assert worst_cancel > 1e4
    t.done()


def test_ln_bwd():
    t = Tally("ln_bwd", tr.LN_BWD_DEFECTS)
    for rows, D, fam in _row_cases():
        g = tr.gen("ln_bwd", rows, D, fam)
        x = tr.row_family(fam, rows, D).to(torch.bfloat16)
        dyg = torch.randn(rows, D, generator=g).to(torch.bfloat16)
        dres = torch.randn(rows, D, generator=g)
        d, e_d, xh, e_xh, _ = tr.ln_bwd_ref(dyg, x, dres)
        got, got_xh = tr.ln_bwd_emul(dyg, x, dres)
        t.clean(got, d, e_d, f"{fam} {rows}x{D}")
        t.clean(got_xh, xh, e_xh, f"x_hat {fam} {rows}x{D}")
        t.case(f"{fam} {rows}x{D}", {df: tr.breaches(tr.ln_bwd_emul(dyg, x, dres, defect=df)[0], d, e_d) for df in tr.LN_BWD_DEFECTS})
        if fam == "benign" and rows == 5:       # the closed form against autograd of LayerNorm (no affine: gamma is folded into dyg)
            xd = x.double().requires_grad_(True)
            torch.nn.functional.layer_norm(xd, (D,), None, None, tr.f32(tr.LN_EPS)).backward(dyg.double())
            assert float((dres.double() + xd.grad - d).abs().max()) < 1e-9 * float(d.abs().max())
    t.done()


def test_small_ln_bwd_and_its_closed_form():
    t = Tally("small_ln_bwd", tr.SMALL_LN_DEFECTS)
    for rows, D in tr.SMALL_LN_SHAPES:
        for fam in tr.SMALL_LN_FAMILIES:
            dy, x, gamma = tr.small_ln_inputs(rows, D, fam)
            d, e_d = tr.small_ln_bwd_ref(dy, x, gamma)
            t.clean(tr.small_ln_bwd_emul(dy, x, gamma), d, e_d, f"{fam} {rows}x{D}")
            t.case(f"{fam} {rows}x{D}", {df: tr.breaches(tr.small_ln_bwd_emul(dy, x, gamma, defect=df), d, e_d) for df in tr.SMALL_LN_DEFECTS})
            dx, _ = tr.ln_rows_autograd(x, dy, gamma)
            assert float((dx - d).abs().max()) <= 1e-9 * float(d.abs().max()) + 1e-12, (fam, rows, D)
    t.done()


def test_embed_bwd_and_its_closed_form():
    t = Tally("embed_bwd", tr.EMBED_DEFECTS)
    for B, np_, Q, D in tr.EMBED_SHAPES:
        ntok = 1 + np_ + Q
        for fam in tr.ROW_FAMILIES:
            X, dY, cls, ctx, gamma = tr.embed_inputs(B, np_, Q, D, fam)
            yx, e_yx, d, e_d, dxp, e_dxp = tr.embed_bwd_ref(X, dY, B, ntok, np_, cls, ctx, gamma)
            what = f"{fam} np {np_} Q {Q} D {D}"
            gx, gd, gp = tr.embed_bwd_emul(X, dY, B, ntok, np_, cls, ctx, gamma)
            t.clean(gx, yx, e_yx, "X " + what)
            t.clean(gd, d, e_d, "dY " + what)
            t.clean(gp, dxp, e_dxp, "patch " + what)
            hits = {}
            for df in tr.EMBED_DEFECTS:
                bx, bd, bp = tr.embed_bwd_emul(X, dY, B, ntok, np_, cls, ctx, gamma, defect=df)
                hits[df] = tr.breaches(bx, yx, e_yx) or tr.breaches(bd, d, e_d) or tr.breaches(bp, dxp, e_dxp)
            t.case(what, hits)
            src = tr.embed_source_rows(X, ntok, np_, cls, ctx)
            dx, dgamma = tr.ln_rows_autograd(src, dY, gamma)
            assert float((dx - d).abs().max()) <= 1e-9 * float(d.abs().max()), what
            assert float((dgamma - yx.sum(0)).abs().max()) <= 1e-9 * float(yx.abs().sum(0).max()), what     # column sums of X_out = d gamma
    t.done()


def test_colsum():
    t = Tally("colsum", tr.COLSUM_DEFECTS)
    for rows, N, lda, fam in tr.colsum_cases():
        for is_f32 in (1, 0):
            A = tr.colsum_input(rows, N, lda, fam, is_f32)
            ref, bound = tr.colsum_ref(A, N)
            what = f"{'f32' if is_f32 else 'bf16'} {fam} {rows}x{N} lda {lda}"
            t.clean(tr.colsum_emul(A, N), ref, bound, what)
            t.case(what, {d: tr.breaches(tr.colsum_emul(A, N, d), ref, bound) for d in tr.COLSUM_DEFECTS})
            if fam == "cancel":      # the bound scales with sum |a|, far above the result
                assert float((bound / ref.abs().clamp_min(1e-30)).min()) > 1e-6 and float(ref.abs().max()) < 1e-2 * float(A[:, :N].double().abs().sum(0).min())
    t.done()


def test_reduce_partials_multi():
    t = Tally("reduce_partials_multi", tr.REDUCE_DEFECTS)
    for njobs, nchunks, n4 in tr.REDUCE_CASES:
        parts = [tr.reduce_input(j, nchunks[j], n4[j]) for j in range(njobs)]
        refs = [tr.reduce_ref(p) for p in parts]
        for j, o in enumerate(tr.reduce_multi_emul(parts)):
            t.clean(o, refs[j][0], refs[j][1], f"job {j} of {nchunks} {n4}")
        hits = {}
        for d in tr.REDUCE_DEFECTS:
            outs = tr.reduce_multi_emul(parts, d)
            hits[d] = any(tr.breaches(o, refs[j][0], refs[j][1]) for j, o in enumerate(outs))
        t.case(f"{nchunks} {n4}", hits)
    t.done()


def test_transposes_are_exact():
    caught = set()
    for R, C in tr.TRANSPOSE_SHAPES:
        for is_f32 in (1, 0):
            src, cs = tr.transpose_input(R, C, C + 8, is_f32)
            for scale in ((cs, None) if is_f32 else (None,)):
                want = tr.transpose_ref(src, C, scale)
                assert want.shape == (C, R) and want.dtype == torch.bfloat16
                assert torch.equal(want.float().t(), (src[:, :C].float() * (scale[None, :] if scale is not None else 1)).to(torch.bfloat16).float())
                hits = {d for d in tr.TRANSPOSE_DEFECTS if not tr.bits_equal(tr.transpose_ref(src, C, scale, d), want)}
                # more than one source row: reading them C apart instead of ld_src apart exists, and must show, in every such case
                assert ("ld_src_ignored" in hits) == (R > 1), (R, C, is_f32, scale is not None)
                caught |= hits
    assert caught == set(tr.TRANSPOSE_DEFECTS)


def _adapter_cases():
    for D, b in tr.ADAPTER_SHAPES:
        for nad in tr.ADAPTER_NAD:
            yield D, b, nad, tr.adapter_numel(D, b)
    yield 128, 8, 3, tr.adapter_numel(128, 8) + 11


def test_adapter_refresh():
    t = Tally("adapter_refresh", tr.REFRESH_DEFECTS)
    for D, b, nad, stride in _adapter_cases():
        assert tr.adapter_numel(D, b) % 2 == 1
        P = tr.adapter_arena(D, b, nad, stride)
        ref = tr.adapter_refresh_ref(P, stride, nad, D, b)
        bp = tr.bpad_of(b)

        def wrong(res):
            bad = False
            for a in range(nad):
                r, e = ref[a], res[a]
                bad |= not all(tr.bits_equal(r[k], e[k]) for k in ("wdf", "up", "upT", "dwgT"))
                bad |= tr.breaches(e["c"], r["c"], r["e_c"]) or tr.breaches(e["d"], r["d"], r["e_d"])
                bad |= bool((e["c"][b:] != 0).any()) or bool((e["d"][b:] != 0).any())
            return bad

        em = tr.adapter_refresh_emul(P, stride, nad, D, b)
        assert not wrong(em)
        for a in range(nad):
            t.clean(em[a]["c"], ref[a]["c"], ref[a]["e_c"], f"c {D} {b}")
            t.clean(em[a]["d"], ref[a]["d"], ref[a]["e_d"], f"d {D} {b}")
            assert ref[a]["wdf"].shape == (bp, D) and ref[a]["up"].shape == (D, bp)
        t.case(f"{D} {b} {nad}", {d: wrong(tr.adapter_refresh_emul(P, stride, nad, D, b, d)) for d in tr.REFRESH_DEFECTS})
    t.done()


def test_adapter_grads_and_their_closed_form():
    t = Tally("adapter_grads", tr.ADAPTER_GRADS_DEFECTS)
    for D, b, nad, stride in _adapter_cases():
        P = tr.adapter_arena(D, b, nad, stride)
        G, cu, T, cd = tr.adapter_grad_operands(P, stride, nad, D, b)
        ref, bound = tr.adapter_grads_ref(G, cu, T, cd, P, stride, nad, D, b)
        t.clean(tr.adapter_grads_emul(G, cu, T, cd, P, stride, nad, D, b), ref, bound, f"{D} {b} {nad}")
        t.case(f"{D} {b} {nad}", {d: tr.breaches(tr.adapter_grads_emul(G, cu, T, cd, P, stride, nad, D, b, d), ref, bound)
                                  for d in tr.ADAPTER_GRADS_DEFECTS})
        for a in range(nad):                 # the two terms of d(scale) are comparable and both far above its bound
            _, _, _, _, uw, ub, _ = tr.adapter_fields(P[a * stride:], D, b)
            t1, t2 = float((G[a, :, :b].double() * uw.double()).sum()), float((cu[a].double() * ub.double()).sum())
            assert 0.1 < abs(t2 / t1) < 10 and abs(t2) > 100 * float(bound[a, -1])
    t.done()
    # closed form == fp64 autograd of the adapter's two linear maps on a small batch
    D, b, m = 128, 8, 19
    g = tr.gen("adapter_autograd")
    P = tr.adapter_arena(D, b, 1, tr.adapter_numel(D, b))
    dH, xh = torch.randn(m, D, generator=g).double(), torch.randn(m, D, generator=g).double()
    dpre, ga = torch.randn(m, b, generator=g).double(), torch.randn(m, b, generator=g).double()
    bp = tr.bpad_of(b)
    G, T, cd = torch.zeros(1, D, bp, dtype=torch.float64), torch.zeros(1, bp, D, dtype=torch.float64), torch.zeros(1, bp, dtype=torch.float64)
    G[0, :, :b], T[0, :b], cd[0, :b] = dH.t() @ ga, dpre.t() @ xh, dpre.sum(0)
    ref, _ = tr.adapter_grads_ref(G, dH.sum(0)[None], T, cd, P, tr.adapter_numel(D, b), 1, D, b)
    want = tr.adapter_grads_autograd(dH, xh, dpre, ga, P, D, b)
    assert float((ref[0] - want).abs().max()) < 1e-10 * float(want.abs().max())


def test_fold_grads_and_their_closed_form():
    t = Tally("fold_grads", tr.FOLD_DEFECTS)
    for D, nparts, re in tr.FOLD_SHAPES:
        T, c, gamma, beta, W = tr.fold_inputs(D, nparts, re)
        dW, e_dW, db, dg, e_dg, dbt, e_dbt = tr.fold_grads_ref(T, c, gamma, beta, W)
        what = f"{D} {nparts}x{re}"

        def wrong(res):
            return (tr.breaches(res[0], dW, e_dW) or not torch.equal(res[1].double(), db) or tr.breaches(res[2], dg, e_dg)
                    or tr.breaches(res[3], dbt, e_dbt))

        em = tr.fold_grads_emul(T, c, gamma, beta, W)
        t.clean(em[0], dW, e_dW, "dW " + what)
        t.clean(em[2], dg, e_dg, "dgamma " + what)
        t.clean(em[3], dbt, e_dbt, "dbeta " + what)
        assert not wrong(em)
        hits = {d: wrong(tr.fold_grads_emul(T, c, gamma, beta, W, d)) for d in tr.FOLD_DEFECTS}
        t.case(what, hits)
        assert hits["dW_without_c_beta"] and hits["dbeta_from_T"]          # these two exist with one row block too
    t.done()
    D, nparts, re, m = 128, 3, 5, 23
    g = tr.gen("fold_autograd")
    _, _, gamma, beta, W = tr.fold_inputs(D, nparts, re)
    xh, dpre = torch.randn(m, D, generator=g).double(), torch.randn(m, nparts * re, generator=g).double()
    dW, _, db, dg, _, dbt, _ = tr.fold_grads_ref(dpre.t() @ xh, dpre.sum(0), gamma, beta, W)
    for got, want in zip((dW, db, dg, dbt), tr.fold_grads_autograd(xh, dpre, gamma, beta, W)):
        assert float((got - want).abs().max()) < 1e-10 * float(want.abs().max())


def test_row_moves_and_row_sums():
    t = Tally("row sums", tr.MOVE_DEFECTS)
    moved = set()
    for B, ntok, Q, D in tr.MOVE_SHAPES:
        g = tr.gen("moves", Q, D)
        dH = torch.randn(B * ntok, D, generator=g)
        ref, bound = tr.concept_rows_sum_ref(dH, B, ntok, Q)
        t.clean(tr.concept_rows_sum_emul(dH, B, ntok, Q), ref, bound, f"concept Q {Q} D {D}")
        t.case(f"concept Q {Q} D {D}", {d: tr.breaches(tr.concept_rows_sum_emul(dH, B, ntok, Q, d), ref, bound) for d in tr.MOVE_DEFECTS})
        nrows = ntok - Q
        ref, bound = tr.token_rows_sum_ref(dH, B, ntok, nrows)
        t.clean(tr.token_rows_sum_emul(dH, B, ntok, nrows), ref, bound, f"token Q {Q} D {D}")
        t.case(f"token Q {Q} D {D}", {d: tr.breaches(tr.token_rows_sum_emul(dH, B, ntok, nrows, d), ref, bound) for d in tr.MOVE_DEFECTS})
        dhf = torch.randn(B * Q, D, generator=g)
        head = torch.randn(B * (1 + Q), D, generator=g)
        # the moves: a row-by-row emulation with the kernels' index arithmetic equals the sliced restatement; shifted by a row it does not
        for kind, src, want in (("scatter", dhf, tr.scatter_concept_rows_ref(dhf, B, ntok, Q)[0]),
                                ("expand", head, tr.expand_head_rows_ref(head, B, ntok, Q)),
                                ("gather", dH, tr.gather_concept_rows_ref(dH, B, ntok, Q))):
            assert tr.bits_equal(tr.row_move_emul(kind, src, B, ntok, Q), want), (kind, Q, D)
            for d in tr.MOVE_DEFECTS:
                assert not tr.bits_equal(tr.row_move_emul(kind, src, B, ntok, Q, d), want), (kind, d, Q, D)
                moved.add(d)
        # the restatements against each other: gather undoes scatter, expand carries the CLS slot
        full, fullb = tr.scatter_concept_rows_ref(dhf, B, ntok, Q)
        assert tr.bits_equal(tr.gather_concept_rows_ref(full, B, ntok, Q), dhf) and tr.bits_equal(fullb, full.to(torch.bfloat16))
        ex = tr.expand_head_rows_ref(head, B, ntok, Q).view(B, ntok, D)
        assert torch.equal(ex[:, 0], head.view(B, 1 + Q, D)[:, 0]) and torch.equal(ex[:, ntok - Q:], head.view(B, 1 + Q, D)[:, 1:])
        assert not bool(ex[:, 1:ntok - Q].any())
    assert moved == set(tr.MOVE_DEFECTS)
    t.done()
