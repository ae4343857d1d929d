"""CPU: the fp64 restatements and derived bounds of tests/forward_kernels_ref.py are (a) finite on every input family, (b) sound -- an fp32
emulation of every operation in ANOTHER summation order stays inside its bound on every input of tests/test_forward_kernels_gpu.py -- and
(c) sharp -- every deliberate defect breaches a bound, or a bit-exact comparison, on at least one of those inputs, and every single case
catches at least one defect (a case whose bound no defect can breach would test nothing).  The worst clean error / bound ratios are
printed (-s)."""
import torch

import forward_kernels_ref as fr
import train_kernels_ref as tr
from test_train_kernels_ref_cpu import Tally


def _ln_cases(Ds):
    return [(rows, D, fam) for D in Ds for rows in fr.LN_ROWS for fam in fr.ROW_FAMILIES]


def test_the_two_pass_bound_does_not_carry_the_one_pass_cancellation():
    """on the offset rows the bound on rstd is near the benign one and four orders of magnitude below the training reference's one-pass
    bound (train_kernels_ref.mean_rstd), whose cancellation factor would let a one-pass kernel through"""
    for D in (128, 384, 1280):
        x = tr.row_family("offset", 37, D)
        _, R, _, e_r = fr.two_pass(x.double(), fr.n_row_stats(D), tr.f32(tr.LN_EPS))
        v = x.double().view(37, D // 64, 64)
        z = torch.zeros(37, D // 64, dtype=torch.float64)
        _, R1, _, e_r1, cancel = tr.mean_rstd(v.sum(-1), (v * v).sum(-1), z, z, D, tr.f32(tr.LN_EPS))
        rel2, rel1 = float((e_r / R).max()), float((e_r1 / R1).max())
        print(f"offset rows D {D}: rstd bound two-pass {rel2:.2e}, one-pass {rel1:.2e} (cancellation factor {float(cancel.max()):.3g})")
        assert rel2 < 1e-3 and rel1 > 20 * rel2 and float(cancel.max()) > 1e4
        # and the one-pass fp32 form really is that much worse than the two-pass form on these rows
        xf = x
        mean = xf.sum(1, keepdim=True) / D
        one = torch.rsqrt(((xf * xf).sum(1, keepdim=True) / D - mean * mean).clamp_min(0) + tr.LN_EPS)
        two = torch.rsqrt(((xf - mean) ** 2).sum(1, keepdim=True) / D + tr.LN_EPS)
        assert float(((two.double() - R).abs() / e_r).max()) <= 1.0
        assert float(((one.double() - R).abs() / e_r).max()) > 1.0


def test_layernorm_fp32_and_bf16_rows():
    """layernorm_f32 (row_stats), the wide bf16 kernel and the generic bf16 kernel: the same operation under three reduction orders"""
    for name, Ds, n_of, in_bf16 in (("layernorm_f32", fr.LN_D_F32, fr.n_row_stats, False), ("layernorm_bf16 wide", fr.LN_D_WIDE, fr.n_wide, True),
                                    ("layernorm_bf16 generic", fr.LN_D_GENERIC + fr.LN_D_RULE, fr.n_row_stats, True)):
        t = Tally(name, fr.LN_DEFECTS)
        for rows, D, fam in _ln_cases(Ds):
            x = tr.row_family(fam, rows, D)
            x = x.to(torch.bfloat16) if in_bf16 else x
            w, b = fr.affine_params(D, "ln")
            ref, bound = fr.layernorm_ref(x, w, b, n_of(D))
            t.clean(fr.layernorm_emul(x, w, b), ref, bound, f"{fam} {rows}x{D}")
            hits = {d: tr.breaches(fr.layernorm_emul(x, w, b, defect=d), ref, bound) for d in fr.LN_DEFECTS}
            if fam == "constant" and rows == 1:
                continue                 # one constant row: the output is the bias under every variance formula but eps outside the root
            t.case(f"{fam} {rows}x{D}", hits)
            if fam == "offset" and rows == 37:
                assert hits["one_pass"], f"{name} D {D}: the offset rows must catch a one-pass variance"
        t.done()


def test_assemble_preln():
    t = Tally("assemble_preln", fr.ASSEMBLE_DEFECTS)
    for B, ntok, np_, D in fr.ASSEMBLE_SHAPES:
        for fam in fr.ROW_FAMILIES:
            H, cls, ctx, pre, ln = fr.assemble_inputs(B, ntok, np_, D, fam)
            y1, e1, y2, e2 = fr.assemble_preln_ref(H, ntok, np_, cls, ctx, pre, ln)
            g1, g2 = fr.assemble_preln_emul(H, ntok, np_, cls, ctx, pre, ln)
            what = f"{fam} {B} {ntok} {np_} {D}"
            t.clean(g1, y1, e1, "H " + what)
            t.clean(g2, y2, e2, "xn " + what)
            hits = {}
            for d in fr.ASSEMBLE_DEFECTS:
                b1, b2 = fr.assemble_preln_emul(H, ntok, np_, cls, ctx, pre, ln, defect=d)
                hits[d] = tr.breaches(b1, y1, e1) or tr.breaches(b2, y2, e2)
            t.case(what, hits)
            # the second bound really carries the first output's error: it is wider than that of the same rows taken as exact inputs
            _, e2_exact = fr.layernorm_ref(y1.float(), ln[0], ln[1], fr.n_row_stats(D))
            assert float((e2 - e2_exact).min()) >= -1e-12 * float(e2.max())
    t.done()


def test_im2col_and_gather_are_exact():
    caught = set()
    for image, patch, Kp in fr.IM2COL_SHAPES:
        for B in fr.IM2COL_B:
            for is_f32 in (1, 0):
                img = fr.im2col_input(B, image, is_f32)
                want = fr.im2col_ref(img, patch, Kp)
                K = 3 * patch * patch
                assert want.shape == (B * (image // patch) ** 2, Kp) and not bool(want[:, K:].float().any())
                assert tr.bits_equal(fr.im2col_emul(img, patch, Kp), want), (image, patch, Kp, B, is_f32)
                hits = {d for d in fr.IM2COL_DEFECTS if not tr.bits_equal(fr.im2col_emul(img, patch, Kp, d), want)}
                assert "kx_ky_swapped" in hits and ("padding_not_zero" in hits) == (Kp > K), (image, patch, Kp, hits)
                caught |= hits
                if not is_f32:           # the bf16 path is a copy: every output value is one of the input's
                    assert tr.bits_equal(want[:, :K].contiguous(), fr.im2col_ref(img.float(), patch, K))
    assert caught == set(fr.IM2COL_DEFECTS)
    for B, ntok, ncon, D in fr.GATHER_SHAPES:
        H = torch.randn(B * ntok, D, generator=fr.gen("gather", B, ntok, ncon, D))
        want = fr.gather_head_rows_ref(H, B, ntok, ncon)
        assert tr.bits_equal(fr.gather_head_rows_emul(H, B, ntok, ncon), want)
        for d in fr.GATHER_DEFECTS:
            assert not tr.bits_equal(fr.gather_head_rows_emul(H, B, ntok, ncon, d), want), (d, B, ntok, ncon)


def test_head():
    t = Tally("head", fr.HEAD_DEFECTS)
    worst = {}
    for D, Q, nbit, B, C, P, ntok in fr.HEAD_SHAPES:
        i = fr.head_inputs(D, Q, nbit, B, C, P, ntok)
        what = f"D {D} Q {Q} nbit {nbit} B {B} C {C} P {P} ntok {ntok}"
        for tag, inputs in (("", i), (" zero BN", fr.head_zero_bn(i))):
            res = fr.head_emul(inputs, B, ntok, Q, nbit)
            codes, e_codes, acc, e_acc = fr.head_codes_ref(inputs, B, ntok, Q, nbit)
            for name, (ref, bound) in (("codes", (codes, e_codes)), ("logits_cont", fr.head_logits_ref(res["codes"], inputs["center_l2"])),
                                       ("logits_bin", fr.head_logits_ref(res["codes"], inputs["center_bin"])),
                                       ("logits_concept", fr.head_concept_ref(inputs, B, ntok, Q)[:2]),
                                       ("image_features", fr.head_image_features_ref(inputs, B, ntok)[:2])):
                r = tr.assert_within(res[name], ref, bound, f"head {name} {what}{tag}", quiet=True)
                worst[name] = max(worst.get(name, 0.0), r)
            assert not fr.head_wrong(res, inputs, B, ntok, Q, nbit)
            if tag:
                assert not bool(res["codes"].any()) and not bool(res["packed"].any()) and not bool(res["logits_cont"].any())
        hits = {d: fr.head_wrong(fr.head_emul(i, B, ntok, Q, nbit, d), i, B, ntok, Q, nbit) for d in fr.HEAD_DEFECTS}
        t.case(what, hits)
        if B >= 5:
            # the special rows do what they are there for: a zero concept row (NaN without the eps), zero codes of both signs (>= packs them)
            assert hits["no_normalize_eps"] and hits["pack_ge"], what
            res = fr.head_emul(i, B, ntok, Q, nbit)
            assert not bool(res["codes"][:, [3, 5]].any())
            sure = acc[:, 5].abs() > e_acc[:, 5]
            assert bool((torch.signbit(res["codes"][:, 5])[sure] == (acc[:, 5] < 0)[sure]).all())
            assert bool(torch.signbit(res["codes"][:, 5]).any()) and not bool(torch.signbit(res["codes"][:, 3]).any()), what + ": no code of -0"
            assert not bool(res["logits_concept"][0, 1].any())
        if B > 1 and Q > 1:
            assert hits["concept_bc_layout"], what
        if B * Q > 1:
            assert hits["row_clamp_off_by_one"], what
    for k, v in worst.items():
        print(f"WORST head {k}: {v:.3f}")
    t.worst = max(worst.values())
    t.done()


def test_pack_codes_words():
    c = torch.zeros(2, 130)
    c[0, [0, 63, 64, 129]] = 1.0
    c[1, 5] = -0.0
    w = fr.pack_codes(c)
    assert w.shape == (2, 3) and w[0].tolist() == [1 - 2 ** 63, 1, 2] and not bool(w[1].any())
    assert fr.pack_codes(c, ge=True)[1].tolist() == [-1, -1, 3]


def test_small_linear():
    t = Tally("small_linear", fr.LINEAR_DEFECTS)
    for rows, in_f, out_f in fr.LINEAR_SHAPES:
        x, W, b = fr.linear_inputs(rows, in_f, out_f)
        hits = {d: False for d in fr.LINEAR_DEFECTS}
        for act in (0, 1):
            for bias in (b, None):
                ref, bound = fr.small_linear_ref(x, W, bias, act)
                t.clean(fr.small_linear_emul(x, W, bias, act), ref, bound, f"{rows} {in_f} {out_f} act {act} bias {bias is not None}")
                for d in fr.LINEAR_DEFECTS:
                    hits[d] |= tr.breaches(fr.small_linear_emul(x, W, bias, act, d), ref, bound)
        t.case(f"{rows} {in_f} {out_f}", hits)
    t.done()


def test_small_layernorm():
    t = Tally("small_layernorm", fr.LN_DEFECTS)
    for D in fr.SMALL_LN_D:
        for rows in fr.SMALL_LN_ROWS:
            for fam in fr.SMALL_LN_FAMILIES:
                x = tr.row_family(fam, rows, D, "small_layernorm")
                w, b = fr.affine_params(D, "small_ln")
                ref, bound = fr.small_layernorm_ref(x, w, b)
                t.clean(fr.ln_f32(x, w, b, tr.LN_EPS), ref, bound, f"{fam} {rows}x{D}")
                t.case(f"{fam} {rows}x{D}", {d: tr.breaches(fr.ln_f32(x, w, b, tr.LN_EPS, d), ref, bound) for d in fr.LN_DEFECTS})
    t.done()


def test_small_mha():
    t = Tally("small_mha", fr.MHA_DEFECTS)
    for T, P, heads in fr.MHA_SHAPES:
        qkv = fr.mha_input(T, P, heads)
        ref, bound = fr.small_mha_ref(qkv, T, P, heads)
        t.clean(fr.small_mha_emul(qkv, T, P, heads), ref, bound, f"{T} {P} {heads}")
        assert float(bound.max()) < 1e-3 * float(qkv[:, 2 * P:].abs().max())            # of fp32 order, far below the softmax's own scale
        if T == 1:                                                                       # one key: the output is v, whatever the scores
            assert torch.equal(fr.small_mha_emul(qkv, T, P, heads), qkv[:, 2 * P:])
        t.case(f"{T} {P} {heads}", {d: tr.breaches(fr.small_mha_emul(qkv, T, P, heads, d), ref, bound) for d in fr.MHA_DEFECTS})
    t.done()


def test_small_l2norm():
    caught = set()
    worst = 0.0
    for rows, cols in fr.L2_SHAPES:
        x = fr.l2_input(rows, cols)
        ref, bound, _, _ = fr.small_l2norm_ref(x)
        l2, bn = fr.small_l2norm_emul(x)
        worst = max(worst, tr.assert_within(l2, ref, bound, f"l2norm {rows}x{cols}", quiet=True))
        assert not fr.l2_wrong(l2, bn, x)
        hits = {d for d in fr.L2_DEFECTS if fr.l2_wrong(*fr.small_l2norm_emul(x, d), x)}
        assert hits, (rows, cols)
        caught |= hits
    print(f"WORST small_l2norm: {worst:.3f}")
    assert caught == set(fr.L2_DEFECTS)


def test_convert_and_add_are_exact():
    for rows, cols, cols_pad in fr.CONVERT_SHAPES:
        x = torch.randn(rows, cols, generator=fr.gen("convert", rows, cols))
        want = fr.convert_bf16_ref(x, cols_pad)
        assert want.shape == (rows, cols_pad) and torch.equal(want[:, :cols].float(), x.to(torch.bfloat16).float()) and not bool(want[:, cols:].float().any())


def test_bn_fold():
    t = Tally("bn_fold", fr.BN_DEFECTS)
    for n in fr.BN_N:
        w, b, mean, var = fr.bn_inputs(n)
        sc, e_sc, sh, e_sh = fr.bn_fold_ref(w, b, mean, var)
        assert float(var.min()) == 0.0
        gs, gh = fr.bn_fold_emul(w, b, mean, var)
        t.clean(gs, sc, e_sc, f"scale {n}")
        t.clean(gh, sh, e_sh, f"shift {n}")
        hits = {}
        for d in fr.BN_DEFECTS:
            bs, bh = fr.bn_fold_emul(w, b, mean, var, defect=d)
            hits[d] = tr.breaches(bs, sc, e_sc) or tr.breaches(bh, sh, e_sh)
        t.case(str(n), hits)
    t.done()


def test_fold_ln():
    t = Tally("fold_ln", fr.FOLD_LN_DEFECTS)
    for b, bpad, D in fr.FOLD_LN_SHAPES:
        Wd, bd, gamma, beta = fr.fold_ln_inputs(b, D)
        wdf, c, e_c, d, e_d = fr.fold_ln_ref(Wd, bd, gamma, beta, bpad)
        em = fr.fold_ln_emul(Wd, bd, gamma, beta, bpad)
        t.clean(em[1], c, e_c, f"c {b} {bpad} {D}")
        t.clean(em[2], d, e_d, f"d {b} {bpad} {D}")
        assert not fr.fold_ln_wrong(em, Wd, bd, gamma, beta, bpad)
        hits = {df: fr.fold_ln_wrong(fr.fold_ln_emul(Wd, bd, gamma, beta, bpad, df), Wd, bd, gamma, beta, bpad) for df in fr.FOLD_LN_DEFECTS}
        t.case(f"{b} {bpad} {D}", hits)
        assert hits["c_unrounded"] and (hits["padding_not_zero"] == (bpad > b))
    t.done()
