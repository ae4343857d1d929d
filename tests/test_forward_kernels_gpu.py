"""GPU: the forward row kernels (rowops.hip), the hashing head (head.hip) and the load-time folds (small_f32.hip), each launched alone
through its tap (include/concepthash_hip_debug.h) and held, element by element, to the fp64 restatement and the bound DERIVED in
tests/forward_kernels_ref.py (nothing tuned to a measured error); copies, single fp32 operations, bf16 conversions and zero padding bit
for bit.  tests/test_forward_kernels_ref_cpu.py shows on the CPU that the bounds are sound and that each deliberate defect breaches them.

The launch discipline is that of tests/kernel_launch.py: every output between sentinel guard blocks and itself the sentinel before the
launch, every input followed by NaN inside its allocation, a second identical launch with identical bytes, the worst error / bound
ratio of every group printed (-s).

Worst error / bound ratios measured on an MI355X (1.0 is the bound; observations, not limits; no kernel breached one, no kernel was changed):
  layernorm_f32 1.000    layernorm_bf16 16-byte kernel 1.000, generic kernel 1.000    assemble_preln H 0.376, xn 0.999
  head codes 0.087, logits_cont 0.113, logits_bin 0.088, logits_concept 0.022, image_features 0.034 (packed codes, hash_features bit-exact)
  small_linear 0.060     small_layernorm 0.586 (the offset rows)     small_mha 0.021     small_l2norm 0.211, |out_bin| 0.153
  bn_fold scale 0.327, shift 0.341        fold_ln c 0.013, d 0.030 (Wdf and the zero rows bit-exact)
  im2col (both input types, fast and slow path, the unaligned image), gather_head_rows, small_add, convert_bf16: bit-exact
A bf16 output sits at 1.000 where the fp32 value falls on a rounding tie (error = the half ulp that IS the bound).
head_dense_kernel: the fp32 MFMA stayed within the any-order fp32 bound gam(D + 1) sum |terms|.  Even the WHOLE error of the two dense
outputs, the error of their left operands included, is below the MFMA's own share of the bound: 0.024 of it for logits_concept, 0.478 for
image_features (whose left operand, the LayerNorm of an offset CLS row, carries most of that error).
The two bf16 LayerNorm kernels against each other, D = 128 and 768, all rows and families: 3 of 192,640 elements differ, each by one bf16
ulp (two half ulps); both kernels are inside the bound at those elements.  Rule 0 equals kernel 1 at D = 1024 and kernel 2 at D = 1280 bit for bit.
"""
import ctypes

import pytest
import torch

import forward_kernels_ref as fr
import train_kernels_ref as tr
from kernel_launch import SENT32, Out, inp, note, report, twice, within

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
_kernel_pair = {"elements": 0, "differ": 0, "max": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from concepthash_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """a HIP error (an illegal access, say) ends the session: nothing more is launched on a device that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after a test, nothing more is launched: {e}", returncode=3)


def _all(shape):
    return torch.ones(shape, dtype=torch.bool)


# ---- LayerNorm rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", fr.LN_D_F32)
def test_layernorm_f32(dev, L, D):
    lib = L.load()
    w, b = fr.affine_params(D, "ln")
    wd, bd = inp(dev, w), inp(dev, b)
    for rows in fr.LN_ROWS:
        for fam in fr.ROW_FAMILIES:
            x = tr.row_family(fam, rows, D)
            ref, bound = fr.layernorm_ref(x, w, b, fr.n_row_stats(D))
            xd = inp(dev, x)

            def launch():
                out = Out(dev, (rows, D), BF16)
                L.check(lib.ch_debug_layernorm_f32(L.ptr(xd), rows, D, L.ptr(wd), L.ptr(bd), tr.LN_EPS, out.ptr, L.stream_ptr()), "layernorm_f32")
                return [out]

            within("layernorm_f32", twice(launch)[0].get(), ref, bound, f"{fam} {rows}x{D}")
    report("layernorm_f32")


@pytest.mark.parametrize("D", sorted(set(fr.LN_D_WIDE + fr.LN_D_GENERIC + fr.LN_D_RULE)))
def test_layernorm_bf16(dev, L, D):
    """kernel 1 (16-byte chunks, D <= 1024) and kernel 2 (generic) each against the bound of its own reduction order; the launcher's rule
    (kernel 0) bit for bit against the kernel it must choose; where both kernels run, how far they differ from each other (printed)"""
    lib = L.load()
    w, b = fr.affine_params(D, "ln")
    wd, bd = inp(dev, w), inp(dev, b)
    kernels = [k for k, Ds in ((1, fr.LN_D_WIDE), (2, fr.LN_D_GENERIC), (0, fr.LN_D_RULE)) if D in Ds]
    for rows in fr.LN_ROWS:
        for fam in fr.ROW_FAMILIES:
            x = tr.row_family(fam, rows, D).to(BF16)
            xd = inp(dev, x)
            got = {}
            for kernel in kernels:
                wide = kernel == 1 or (kernel == 0 and D <= 1024)
                ref, bound = fr.layernorm_ref(x, w, b, fr.n_wide(D) if wide else fr.n_row_stats(D))

                def launch():
                    out = Out(dev, (rows, D), BF16)
                    L.check(lib.ch_debug_layernorm_bf16(L.ptr(xd), rows, D, L.ptr(wd), L.ptr(bd), tr.LN_EPS, out.ptr, kernel, L.stream_ptr()),
                            "layernorm_bf16")
                    return [out]

                got[kernel] = twice(launch)[0].get()
                within(f"layernorm_bf16 {'wide' if wide else 'generic'}", got[kernel], ref, bound, f"{fam} {rows}x{D} kernel {kernel}")
            if 0 in got:
                same = 1 if D <= 1024 else 2
                if same in got:
                    assert tr.bits_equal(got[0], got[same]), f"{fam} {rows}x{D}: the launcher's rule did not run kernel {same}"
            if 1 in got and 2 in got:
                diff = (got[1].double() - got[2].double()).abs()
                _kernel_pair["elements"] += diff.numel()
                _kernel_pair["differ"] += int((diff > 0).sum())
                _kernel_pair["max"] = max(_kernel_pair["max"], float((diff / tr.half_ulp_bf16(got[2].double().abs())).max()))
    report("layernorm_bf16 wide", "layernorm_bf16 generic")
    print(f"KERNEL PAIR wide vs generic so far: {_kernel_pair['differ']} of {_kernel_pair['elements']} elements differ, "
          f"by at most {_kernel_pair['max']:.1f} half ulps of bf16")


def test_layernorm_bf16_rule_against_both_kernels(dev, L):
    """D = 1024 is the last width of the 16-byte kernel and 1280 the first of the generic one: rule 0 equals kernel 1 / kernel 2 bit for bit
    there, and the 16-byte kernel refuses 1280 without writing anything"""
    lib = L.load()
    rows = 5
    for D, same in ((1024, 1), (1280, 2)):
        w, b = fr.affine_params(D, "ln")
        wd, bd = inp(dev, w), inp(dev, b)
        xd = inp(dev, tr.row_family("benign", rows, D).to(BF16))
        outs = []
        for kernel in (0, same):
            out = Out(dev, (rows, D), BF16)
            L.check(lib.ch_debug_layernorm_bf16(L.ptr(xd), rows, D, L.ptr(wd), L.ptr(bd), tr.LN_EPS, out.ptr, kernel, L.stream_ptr()), "layernorm_bf16")
            torch.cuda.synchronize()
            outs.append(out.get())
        assert tr.bits_equal(outs[0], outs[1]), f"D {D}: rule 0 is not kernel {same}"
    for D, kernel in ((1280, 1), (128, 3)):
        w, b = fr.affine_params(D, "ln")
        wd, bd = inp(dev, w), inp(dev, b)
        xd = inp(dev, tr.row_family("benign", rows, D).to(BF16))
        out = Out(dev, (rows, D), BF16)
        assert lib.ch_debug_layernorm_bf16(L.ptr(xd), rows, D, L.ptr(wd), L.ptr(bd), tr.LN_EPS, out.ptr, kernel, L.stream_ptr()) != 0
        torch.cuda.synchronize()
        assert out.untouched(_all((rows, D)))


@pytest.mark.parametrize("B,ntok,np_,D", fr.ASSEMBLE_SHAPES)
def test_assemble_preln(dev, L, B, ntok, np_, D):
    lib = L.load()
    for fam in fr.ROW_FAMILIES:
        H, cls, ctx, pre, ln = fr.assemble_inputs(B, ntok, np_, D, fam)
        y1, e1, y2, e2 = fr.assemble_preln_ref(H, ntok, np_, cls, ctx, pre, ln)
        t = torch.arange(B * ntok) % ntok
        Hs = H.clone().view(torch.int32)
        Hs[(t == 0) | (t > np_)] = SENT32                   # the rows the kernel takes from cls_pos0 / ctx hold the sentinel, not a value
        cd, xd = inp(dev, cls), inp(dev, ctx)
        pd = [inp(dev, v) for v in pre + ln]

        def launch():
            oH, oX = Out(dev, (B * ntok, D), F32, init=Hs.view(F32)), Out(dev, (B * ntok, D), BF16)
            L.check(lib.ch_debug_assemble_preln(oH.ptr, B, ntok, np_, D, L.ptr(cd), L.ptr(xd), L.ptr(pd[0]), L.ptr(pd[1]), L.ptr(pd[2]), L.ptr(pd[3]),
                                                tr.LN_EPS, oX.ptr, L.stream_ptr()), "assemble_preln")
            return [oH, oX]

        oH, oX = twice(launch)
        within("assemble_preln H", oH.get(), y1, e1, f"{fam} {B} {ntok} {np_} {D}")
        within("assemble_preln xn", oX.get(), y2, e2, f"{fam} {B} {ntok} {np_} {D}")
    report("assemble_preln H", "assemble_preln xn")


# ---- im2col, gather_head_rows: bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image,patch,Kp", fr.IM2COL_SHAPES)
def test_im2col(dev, L, image, patch, Kp):
    lib = L.load()
    for B in fr.IM2COL_B:
        for is_f32 in (1, 0):
            img = fr.im2col_input(B, image, is_f32)
            want = fr.im2col_ref(img, patch, Kp)
            shifts = (0, 1) if (image, patch, Kp) == fr.IM2COL_SHAPES[0] else (0,)
            for shift in shifts:                             # shift 1: the image starts one element into its allocation (not 16-byte aligned)
                flat = torch.cat([torch.full((shift,), float("nan"), dtype=img.dtype), img.reshape(-1)])
                fd = inp(dev, flat)
                p_img = ctypes.c_void_p(fd.data_ptr() + shift * fd.element_size())
                assert (p_img.value % 16 == 0) == (shift == 0)

                def launch():
                    out = Out(dev, want.shape, BF16)
                    L.check(lib.ch_debug_im2col(p_img, 0 if is_f32 else 1, B, image, patch, Kp, out.ptr, L.stream_ptr()), "im2col")
                    return [out]

                got = twice(launch)[0].get()
                assert tr.bits_equal(got, want), f"im2col image {image} patch {patch} Kp {Kp} B {B} {'f32' if is_f32 else 'bf16'} shift {shift}"


@pytest.mark.parametrize("B,ntok,ncon,D", fr.GATHER_SHAPES)
def test_gather_head_rows(dev, L, B, ntok, ncon, D):
    lib = L.load()
    H = torch.randn(B * ntok, D, generator=fr.gen("gather", B, ntok, ncon, D))
    Hd = inp(dev, H)

    def launch():
        out = Out(dev, (B * (1 + ncon), D), F32)
        L.check(lib.ch_debug_gather_head_rows(L.ptr(Hd), B, ntok, ncon, D, out.ptr, L.stream_ptr()), "gather_head_rows")
        return [out]

    assert tr.bits_equal(twice(launch)[0].get(), fr.gather_head_rows_ref(H, B, ntok, ncon))


# ---- the hashing head -------------------------------------------------------------------------------------------------------------------------
_HEAD_IN = ("hash_pe", "hash_fc", "bn_scale", "bn_shift", "center_l2", "center_bin", "concept_pe", "concept_cent_l2", "post_w", "post_b", "vis_proj")


def _head_launch(dev, L, d, dims, want):
    """one ch_debug_head on the device inputs d; `want`: the optional outputs to ask for.  Returns (status, {name: Out})"""
    D, Q, nbit, B, C, P, ntok = dims
    shapes = dict(codes=((B, nbit), F32), packed=((B, fr.cdiv(nbit, 64)), torch.int64), logits_cont=((B, C), F32), logits_bin=((B, C), F32),
                  logits_concept=((Q, B, C), F32), hash_features=((B, Q, D), F32), image_features=((B, P), F32))
    o = {k: Out(dev, *shapes[k]) for k in ("codes",) + tuple(want)}
    p = lambda k: o[k].ptr if k in o else None
    st = L.load().ch_debug_head(L.ptr(d["H"]), B, ntok, D, Q, nbit, C, P, *[L.ptr(d[k]) for k in _HEAD_IN], tr.LN_EPS, p("codes"), p("packed"),
                                p("logits_cont"), p("logits_bin"), p("logits_concept"), p("hash_features"), p("image_features"), L.stream_ptr())
    return st, o


def _head_check(o, i, dims, what):
    D, Q, nbit, B, C, P, ntok = dims
    codes = o["codes"].get()
    ref, bound, acc, e_acc = fr.head_codes_ref(i, B, ntok, Q, nbit)
    within("head codes", codes, ref, bound, what)
    if "packed" in o:
        assert torch.equal(o["packed"].get(), fr.pack_codes(codes)), what + ": out_packed is not (out_codes > 0)"
    if "logits_cont" in o:
        within("head logits_cont", o["logits_cont"].get(), *fr.head_logits_ref(codes, i["center_l2"]), what)
    if "logits_bin" in o:
        within("head logits_bin", o["logits_bin"].get(), *fr.head_logits_ref(codes, i["center_bin"]), what)
    if "logits_concept" in o:
        got = o["logits_concept"].get()
        ref, bound, dense = fr.head_concept_ref(i, B, ntok, Q)
        within("head logits_concept", got, ref, bound, what)
        note("head logits_concept, whole error over the MFMA's any-order share alone", float(((got.double() - ref).abs() / dense).max()))
    if "hash_features" in o:
        assert tr.bits_equal(o["hash_features"].get(), fr._hash_rows(i["H"], B, ntok, Q).contiguous()), what + ": hash_features is not a copy"
    if "image_features" in o:
        got = o["image_features"].get()
        ref, bound, dense = fr.head_image_features_ref(i, B, ntok)
        within("head image_features", got, ref, bound, what)
        note("head image_features, whole error over the MFMA's any-order share alone", float(((got.double() - ref).abs() / dense).max()))
    return codes, acc, e_acc


@pytest.mark.parametrize("D,Q,nbit,B,C,P,ntok", fr.HEAD_SHAPES)
def test_head(dev, L, D, Q, nbit, B, C, P, ntok):
    """output sets: the codes alone, each optional output alone, all together; then all together with every BN constant zero"""
    dims = (D, Q, nbit, B, C, P, ntok)
    i = fr.head_inputs(*dims)
    what = f"D {D} Q {Q} nbit {nbit} B {B} C {C} P {P} ntok {ntok}"
    for tag, inputs, sets in (("", i, [()] + [(k,) for k in fr.HEAD_OUTPUTS] + [fr.HEAD_OUTPUTS]), (" zero BN", fr.head_zero_bn(i), [fr.HEAD_OUTPUTS])):
        d = {k: inp(dev, v) for k, v in inputs.items()}
        for want in sets:
            def launch():
                st, o = _head_launch(dev, L, d, dims, want)
                L.check(st, "head")
                launch.names = list(o)
                return list(o.values())

            outs = twice(launch)
            o = dict(zip(launch.names, outs))
            codes, acc, e_acc = _head_check(o, inputs, dims, f"{what}{tag} outputs {'+'.join(want) or 'codes'}")
            if tag:
                assert not bool(codes.any()), what + ": zero BN constants must give zero codes"
                if "packed" in o:
                    assert not bool(o["packed"].get().any()) and not bool(o["logits_cont"].get().any()) and not bool(o["logits_bin"].get().any())
            elif B >= 5:
                assert not bool(codes[:, [3, 5]].any()), what + ": bn_scale = 0 with bn_shift = +-0 must give a zero code"
                sure = acc[:, 5].abs() > e_acc[:, 5]
                assert bool((torch.signbit(codes[:, 5])[sure] == (acc[:, 5] < 0)[sure]).all()) and bool(torch.signbit(codes[:, 5]).any())
                assert not bool(torch.signbit(codes[:, 3]).any())
                if "logits_concept" in o:
                    assert not bool(o["logits_concept"].get()[0, 1].any()), what + ": a zero concept row must give zero logits (F.normalize eps)"
    report("head codes", "head logits_cont", "head logits_bin", "head logits_concept", "head image_features",
           "head logits_concept, whole error over the MFMA's any-order share alone", "head image_features, whole error over the MFMA's any-order share alone")


@pytest.mark.parametrize("case", fr.HEAD_REFUSALS)
def test_head_refusals(dev, L, case):
    """nbit % Q != 0, D % 16 != 0, Q D floats past the 64 KiB of LDS: a status from the host-side checks, nothing launched, nothing written"""
    D, Q, nbit = case["D"], case["Q"], case["nbit"]
    dims = (D, Q, nbit, 2, 3, 16, Q + 1)
    g = fr.gen("head_refusal", D, Q, nbit)
    sub = fr.cdiv(nbit, Q)
    shapes = dict(H=(2 * (Q + 1), D), hash_pe=(Q, D), hash_fc=(sub, D), bn_scale=(nbit,), bn_shift=(nbit,), center_l2=(3, nbit), center_bin=(3, nbit),
                  concept_pe=(Q, D), concept_cent_l2=(3, D), post_w=(D,), post_b=(D,), vis_proj=(16, D))
    d = {k: inp(dev, torch.randn(*s, generator=g)) for k, s in shapes.items()}
    st, o = _head_launch(dev, L, d, dims, fr.HEAD_OUTPUTS)
    torch.cuda.synchronize()
    assert st != 0 and L.load().ch_last_error()
    for k, out in o.items():
        assert out.untouched(_all(out.shape)), f"{k} was written by a refused call"


# ---- load-time folds --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,in_f,out_f", fr.LINEAR_SHAPES)
def test_small_linear(dev, L, rows, in_f, out_f):
    lib = L.load()
    x, W, b = fr.linear_inputs(rows, in_f, out_f)
    xd, Wd, bd = inp(dev, x), inp(dev, W), inp(dev, b)
    for act in (0, 1):
        for bias in (b, None):
            ref, bound = fr.small_linear_ref(x, W, bias, act)

            def launch():
                out = Out(dev, (rows, out_f), F32)
                L.check(lib.ch_debug_small_linear(L.ptr(xd), rows, in_f, L.ptr(Wd), L.ptr(bd) if bias is not None else None, out_f, act, out.ptr,
                                                  L.stream_ptr()), "small_linear")
                return [out]

            got = twice(launch)[0].get()
            within("small_linear", got, ref, bound, f"{rows} {in_f} {out_f} act {act} bias {bias is not None}")
            if act == 1:
                assert bool((got >= 0).all())
    report("small_linear")


@pytest.mark.parametrize("D", fr.SMALL_LN_D)
def test_small_layernorm(dev, L, D):
    lib = L.load()
    w, b = fr.affine_params(D, "small_ln")
    wd, bd = inp(dev, w), inp(dev, b)
    for rows in fr.SMALL_LN_ROWS:
        for fam in fr.SMALL_LN_FAMILIES:
            x = tr.row_family(fam, rows, D, "small_layernorm")
            ref, bound = fr.small_layernorm_ref(x, w, b)
            xd = inp(dev, x)

            def launch():
                out = Out(dev, (rows, D), F32)
                L.check(lib.ch_debug_small_layernorm(L.ptr(xd), rows, D, L.ptr(wd), L.ptr(bd), tr.LN_EPS, out.ptr, L.stream_ptr()), "small_layernorm")
                return [out]

            within("small_layernorm", twice(launch)[0].get(), ref, bound, f"{fam} {rows}x{D}")
    report("small_layernorm")


@pytest.mark.parametrize("n", fr.ADD_N)
def test_small_add(dev, L, n):
    lib = L.load()
    g = fr.gen("small_add", n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
    ad, bd = inp(dev, a), inp(dev, b)

    def launch():
        out = Out(dev, (n,), F32)
        L.check(lib.ch_debug_small_add(L.ptr(ad), L.ptr(bd), n, out.ptr, L.stream_ptr()), "small_add")
        return [out]

    assert tr.bits_equal(twice(launch)[0].get(), a + b), "small_add is one fp32 addition"


@pytest.mark.parametrize("T,P,heads", fr.MHA_SHAPES)
def test_small_mha(dev, L, T, P, heads):
    lib = L.load()
    qkv = fr.mha_input(T, P, heads)
    ref, bound = fr.small_mha_ref(qkv, T, P, heads)
    qd = inp(dev, qkv)

    def launch():
        out = Out(dev, (T, P), F32)
        L.check(lib.ch_debug_small_mha(L.ptr(qd), T, P, heads, out.ptr, L.stream_ptr()), "small_mha")
        return [out]

    within("small_mha", twice(launch)[0].get(), ref, bound, f"{T} {P} {heads}")
    report("small_mha")


@pytest.mark.parametrize("rows,cols", fr.L2_SHAPES)
def test_small_l2norm(dev, L, rows, cols):
    lib = L.load()
    x = fr.l2_input(rows, cols)
    ref, bound, bs, e_bs = fr.small_l2norm_ref(x)
    xd = inp(dev, x)
    for with_bin in (True, False):
        def launch():
            o = [Out(dev, (rows, cols), F32)] + ([Out(dev, (rows, cols), F32)] if with_bin else [])
            L.check(lib.ch_debug_small_l2norm(L.ptr(xd), rows, cols, o[0].ptr, o[1].ptr if with_bin else None, L.stream_ptr()), "small_l2norm")
            return o

        o = twice(launch)
        l2 = o[0].get()
        within("small_l2norm", l2, ref, bound, f"{rows}x{cols} out_bin {with_bin}")
        if rows > 1:
            assert not bool(l2[0].any()), "a zero row must give zeros"
        if with_bin:
            bn = o[1].get()
            assert torch.equal(torch.sign(bn), torch.sign(l2)), "out_bin's signs are not those of out_l2"
            nz = bn != 0
            note("small_l2norm bin", float(((bn.double().abs() - bs).abs()[nz] / e_bs).max()))
            assert bool(((bn.double().abs() - bs).abs()[nz] <= e_bs).all()), "|out_bin| is not cols^-1/2"
    report("small_l2norm", "small_l2norm bin")


@pytest.mark.parametrize("rows,cols,cols_pad", fr.CONVERT_SHAPES)
def test_convert_bf16(dev, L, rows, cols, cols_pad):
    lib = L.load()
    x = torch.randn(rows, cols, generator=fr.gen("convert", rows, cols))
    xd = inp(dev, x)

    def launch():
        out = Out(dev, (rows, cols_pad), BF16)
        L.check(lib.ch_debug_convert_bf16(L.ptr(xd), rows, cols, cols_pad, out.ptr, L.stream_ptr()), "convert_bf16")
        return [out]

    assert tr.bits_equal(twice(launch)[0].get(), fr.convert_bf16_ref(x, cols_pad))


@pytest.mark.parametrize("n", fr.BN_N)
def test_bn_fold(dev, L, n):
    lib = L.load()
    w, b, mean, var = fr.bn_inputs(n)
    sc, e_sc, sh, e_sh = fr.bn_fold_ref(w, b, mean, var)
    d = [inp(dev, v) for v in (w, b, mean, var)]

    def launch():
        o = [Out(dev, (n,), F32), Out(dev, (n,), F32)]
        L.check(lib.ch_debug_bn_fold(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), n, fr.BN_EPS, o[0].ptr, o[1].ptr, L.stream_ptr()), "bn_fold")
        return o

    o = twice(launch)
    within("bn_fold scale", o[0].get(), sc, e_sc, str(n))
    within("bn_fold shift", o[1].get(), sh, e_sh, str(n))
    report("bn_fold scale", "bn_fold shift")


@pytest.mark.parametrize("b,bpad,D", fr.FOLD_LN_SHAPES)
def test_fold_ln(dev, L, b, bpad, D):
    lib = L.load()
    Wd, bd, gamma, beta = fr.fold_ln_inputs(b, D)
    wdf, c, e_c, d, e_d = fr.fold_ln_ref(Wd, bd, gamma, beta, bpad)
    dd = [inp(dev, v) for v in (Wd, bd, gamma, beta)]

    def launch():
        o = [Out(dev, (bpad, D), BF16), Out(dev, (bpad,), F32), Out(dev, (bpad,), F32)]
        L.check(lib.ch_debug_fold_ln(L.ptr(dd[0]), L.ptr(dd[1]), L.ptr(dd[2]), L.ptr(dd[3]), b, bpad, D, o[0].ptr, o[1].ptr, o[2].ptr, L.stream_ptr()),
                "fold_ln")
        return o

    o = twice(launch)
    what = f"b {b} bpad {bpad} D {D}"
    assert tr.bits_equal(o[0].get()[:b].contiguous(), wdf[:b].contiguous()), what + ": Wdf is not bf16(Wd * gamma)"
    assert not bool(o[0].get()[b:].float().any()), what + ": Wdf rows past b must be zero"
    within("fold_ln c", o[1].get(), c, e_c, what)
    within("fold_ln d", o[2].get(), d, e_d, what)
    assert not bool(o[1].get()[b:].any()) and not bool(o[2].get()[b:].any()), what + ": c / d past b must be zero"
    report("fold_ln c", "fold_ln d")
