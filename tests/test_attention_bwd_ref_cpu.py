"""CPU: the fp64 attention-backward reference, its derived error bounds, its cotangent builders and its emulation
(tests/attention_bwd_ref.py) are sound before tests/test_attention_bwd_gpu.py holds the two backward kernels to them:
  * the closed form equals fp64 autograd;
  * a torch emulation of either kernel's arithmetic stays inside the bound on the builders, lengths and concept-token counts the GPU
    file uses (the worst error / bound ratio per group is printed: the bound is neither vacuous nor broken).  Left out here to keep
    this file under a minute, and run on the GPU only: the streaming lengths 1024, 1088 and 1089;
  * the builders deliver what they promise;
  * the emulation with each deliberate defect fails the very assertion helper the GPU tests call, at the smallest length and concept
    count where the defect can act, on inputs the GPU file runs at that length."""
import pytest
import torch

import attention_bwd_ref as br

B, H = br.B_TEST, br.H_TEST
CPU_STREAM = tuple(n for n in br.STREAM_LENGTHS if n <= 320)
_worst = {}


def _check(group, name, do_name, n, ncon=0, ext_name=None, streaming=False):
    qkv = br.build(name, B, n, H)
    dO = br.build_do(do_name, B, n, H)
    ext = br.build_ext(ext_name, B, n, H, ncon) if ext_name else None
    ref, bound = br.bounds(qkv, dO, ext, B, n, H, ncon=ncon, streaming=streaming)
    got = br.emulate(qkv, dO, ext, B, n, H, ncon=ncon, streaming=streaming)
    r = br.assert_all_within(got, ref, bound, f"{group} {name} dO {do_name} ext {ext_name} {n} tokens ncon {ncon}")
    _worst[group] = tuple(max(a, b) for a, b in zip(_worst.get(group, (0.0, 0.0, 0.0)), r))
    if n == 1:                                                     # one key: P = 1, dS = 0, dV = dO exactly
        D = H * 64
        assert not bool(got[:, :2 * D].float().any()) and torch.equal(got[:, 2 * D:], dO)
    return r


def _report(group):
    w = _worst[group]
    print(f"WORST {group}: dq {w[0]:.3f} dk {w[1]:.3f} dv {w[2]:.3f}")
    assert min(w) > 0.02, (group, w)                               # not vacuous: the emulation uses a visible part of every bound


@pytest.mark.parametrize("name", br.BUILDERS)
def test_emulation_within_bound_resident(name):
    group = f"resident {name}"
    for n in br.RESIDENT_LENGTHS:
        for do_name in ("benign", "one_row"):
            _check(group, name, do_name, n)
    for n in br.SCALED_LENGTHS:
        _check(group, name, "scaled", n)
    _report(group)


@pytest.mark.parametrize("ext_name", br.EXT_BUILDERS)
def test_emulation_within_bound_resident_ext(ext_name):
    group = f"resident ext {ext_name}"
    for ncon in br.TAP_NCON:
        for n in br.ext_lengths(ncon):
            for name in br.TAP_BUILDERS:
                _check(group, name, "benign", n, ncon=ncon, ext_name=ext_name)
    _report(group)


@pytest.mark.parametrize("name", br.STREAM_BUILDERS)
def test_emulation_within_bound_streaming(name):
    group = f"streaming {name}"
    for n in CPU_STREAM:
        _check(group, name, "benign", n, streaming=True)
        if n >= br.STREAM_NCON + 2:
            _check(group, name, "benign", n, ncon=br.STREAM_NCON, ext_name="benign", streaming=True)
    _report(group)


def test_emulation_within_bound_streaming_ncon_edges():
    group = "streaming ncon edges"
    for n in br.STREAM_NCON_LENGTHS:
        for ncon in br.STREAM_NCON_EDGE:
            for ext_name in br.EXT_BUILDERS:
                _check(group, "benign", "benign", n, ncon=ncon, ext_name=ext_name, streaming=True)
    _report(group)


def test_closed_form_equals_autograd():
    for name, do_name, n, ncon, ext_name in (("benign", "benign", 1, 0, None), ("benign", "scaled", 17, 0, None), ("peaked", "one_row", 65, 0, None),
                                             ("offset", "benign", 33, 0, None), ("benign", "benign", 3, 1, "corners"),
                                             ("peaked", "benign", 37, 4, "benign"), ("last_key", "benign", 129, 17, "corners")):
        qkv, dO = br.build(name, B, n, H), br.build_do(do_name, B, n, H)
        ext = br.build_ext(ext_name, B, n, H, ncon) if ext_name else None
        a, b = br.closed_form(qkv, dO, ext, B, n, H, ncon), br.autograd(qkv, dO, ext, B, n, H, ncon)
        scale = float(b.abs().max()) + 1e-300
        assert float((a - b).abs().max()) <= 1e-12 * scale, (name, n, float((a - b).abs().max()), scale)
        ref, _ = br.bounds(qkv, dO, ext, B, n, H, ncon=ncon)
        assert float((ref - b).abs().max()) <= 1e-12 * scale, (name, n)       # and bounds() returns the same reference


def test_builders_deliver_what_they_promise():
    for n in (1, 2, 17, 288):
        D = H * 64
        x = br.build_do("one_row", B, n, H).float().view(B, n, D)
        for b in range(B):
            row = n - 1 if b % 2 == 0 else 0
            nz = x[b].abs().sum(-1) > 0
            assert int(nz.sum()) == 1 and bool(nz[row]), (n, b)                 # exactly one non-zero row, where promised
        if B >= 2 and n >= 2:
            assert bool(x[0, n - 1].any()) and bool(x[1, 0].any())              # both the last token and token 0 occur
    for n in br.SCALED_LENGTHS:
        mag = br.build_do("scaled", B, n, H).float().view(B * n, -1).pow(2).mean(-1).sqrt()
        assert float(mag.min()) < 2.0 ** -5 and float(mag.max()) > 2.0 ** 5, (n, float(mag.min()), float(mag.max()))
        assert float(mag.log2().std()) > 2.5, n                                 # spread, not two clusters
    assert torch.equal(br.build_do("benign", B, 17, H), br.build_do("benign", B, 17, H))       # seeded
    for ncon, n in ((1, 3), (4, 36), (64, 288)):
        np_ = n - ncon - 1
        e = br.build_ext("corners", B, n, H, ncon)
        assert e.shape == (B, H, ncon, np_)
        want = {(0, 0), (0, np_ - 1), (ncon - 1, 0), (ncon - 1, np_ - 1)}
        nz = {(int(r), int(c)) for r, c in torch.nonzero(e[0, 0])}
        assert nz == want and bool((e[0, 0][e[0, 0] != 0].abs() == br.CORNER).all()), (ncon, n, nz)   # also where corners coincide
        b_ = br.build_ext("benign", B, n, H, ncon)
        assert b_.shape == e.shape and 2.0 < float(b_.std()) < 4.0 or b_.numel() < 64


def _fails(defect, name, do_name, n, ncon=0, ext_name=None, streaming=False):
    qkv, dO = br.build(name, B, n, H), br.build_do(do_name, B, n, H)
    ext = br.build_ext(ext_name, B, n, H, ncon) if ext_name else None
    ref, bound = br.bounds(qkv, dO, ext, B, n, H, ncon=ncon, streaming=streaming)
    got = br.emulate(qkv, dO, ext, B, n, H, ncon=ncon, streaming=streaming, defect=defect)
    try:
        br.assert_all_within(got, ref, bound, f"defect {defect} {name} {do_name} {ext_name} {n} ncon {ncon}")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("streaming", [False, True])
def test_deliberate_defects_breach_the_bound(streaming):
    """Every defect fails br.assert_all_within at the smallest length / concept count where it can act (and at larger ones), on a case
    of the GPU file: resident lengths 1, 2, 3 (= ncon + 2 for ncon = 1), 17, 35-37, 288; streaming 63, 65, 129, 320."""
    kw = dict(streaming=streaming)
    small = (63, 65, 129) if streaming else (2, 17, 288)
    for n in small:
        assert _fails("drop_last_key", "last_key", "benign", n, **kw), n
        assert _fails("dup_last_key", "last_key", "benign", n, **kw), n
        assert _fails("dup_last_query", "benign", "one_row", n, **kw), n
        assert _fails("dup_last_query", "benign", "benign", n, **kw), n
    if not streaming:
        assert _fails("dup_last_key", "benign", "benign", 1), 1                 # two copies of the only key: lse grows by 1, dv halves
        assert _fails("dup_last_query", "benign", "one_row", 1), 1
    # the smallest problem with ext: ncon = 1, n = 3 (resident; the GPU file runs it), ncon = 1 at 129 (streaming)
    cases = ((1, 129), (4, 129), (17, 320)) if streaming else ((1, 3), (4, 6), (4, 36), (16, 201), (64, 288))
    for ncon, n in cases:
        for defect in ("ext_phase_a_only", "ext_phase_b_only", "ext_key_shift", "ext_query_shift", "dq_from_o"):
            assert _fails(defect, "benign", "benign", n, ncon=ncon, ext_name="corners", **kw), (defect, ncon, n)
            if defect in ("ext_phase_a_only", "ext_phase_b_only", "ext_query_shift"):
                assert _fails(defect, "benign", "benign", n, ncon=ncon, ext_name="benign", **kw), (defect, ncon, n)
    if streaming:
        for n in (65, 129, 320):                                               # two blocks: the first length with a rescale
            assert _fails("no_pd_rescale", "ascending", "benign", n, **kw), n
        for n in (129, 320):                                                   # three blocks: the first length where a stage is reused
            assert _fails("stale_block", "benign", "benign", n, **kw), n
            assert _fails("stale_block", "descending", "benign", n, **kw), n    # (ascending would hide it: early blocks weigh e^-8 of the last)
    # and without a defect the same calls pass
    assert not _fails(None, "last_key", "benign", small[1], **kw)
    assert not _fails(None, "benign", "one_row", small[1], **kw)
    assert not _fails(None, "benign", "benign", cases[0][1], ncon=cases[0][0], ext_name="corners", **kw)
