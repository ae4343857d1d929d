"""CPU: the fp64 attention reference, its derived error bound and its input builders (tests/attention_ref.py) are sound before
tests/test_attention_fwd_gpu.py holds the kernels to them:
  * a torch emulation of the kernels' arithmetic stays inside the bound on every builder and length the GPU tests use (the worst
    error / bound ratio is printed: the bound is neither vacuous nor broken);
  * the builders produce what they promise (a last key that carries real mass, peaked rows, large common offsets, a running maximum
    that rises in every block / is fixed by the first block);
  * the emulation with a deliberate defect -- last key dropped or counted twice, causal mask off by one either way, tapped range
    shifted by one -- fails the very assertion helper the GPU tests call."""
import pytest
import torch

import attention_ref as ar

B, H = ar.B_TEST, ar.H_TEST


def _check(name, n, causal=False, streaming=False, ncon=0):
    qkv = ar.build(name, B, n, H)
    ref, bound, p, p_bound = ar.bounds(qkv, B, n, H, causal=causal, streaming=streaming)
    tap_on = ncon and n >= ncon + 2
    out, tap = ar.emulate(qkv, B, n, H, causal=causal, streaming=streaming, ncon=ncon if tap_on else 0)
    what = f"{'streaming' if streaming else 'causal' if causal else 'resident'} {name} {n} tokens"
    r = ar.assert_within(out, ref, bound, what)
    assert r > 0.02 or n == 1, (what, r)                          # not vacuous: the emulation uses a visible part of the bound
    if tap_on:
        ar.assert_within(tap, ar.tapped(p, ncon), ar.tapped(p_bound, ncon), what + f" tap ncon {ncon}")
    if n == 1 or causal:                                          # one visible key: the output IS v (row 0 of every sequence when causal)
        v = qkv.view(B, n, 3, H, 64)[:, 0, 2].reshape(B, H * 64)
        assert torch.equal(out.view(B, n, H * 64)[:, 0], v)


@pytest.mark.parametrize("name", ar.BUILDERS)
def test_emulation_within_bound_resident(name):
    for n in ar.RESIDENT_LENGTHS:
        _check(name, n)


@pytest.mark.parametrize("name", ar.TAP_BUILDERS)
def test_emulation_within_bound_tap(name):
    for ncon in ar.TAP_NCON:
        for n in ar.tap_lengths(ncon):
            _check(name, n, ncon=ncon)


@pytest.mark.parametrize("name", ar.CAUSAL_BUILDERS)
def test_emulation_within_bound_causal(name):
    for n in ar.CAUSAL_LENGTHS:
        _check(name, n, causal=True)


@pytest.mark.parametrize("name", ar.STREAM_BUILDERS)
def test_emulation_within_bound_streaming(name):
    for n in ar.STREAM_LENGTHS:
        _check(name, n, streaming=True, ncon=ar.STREAM_NCON)
    _check(name, ar.STREAM_MAX[0], streaming=True, ncon=ar.STREAM_MAX[1])


def _scaled_logits(qkv, n):
    q, k, _ = ar.split(qkv, B, n, H)
    return q @ k.transpose(-1, -2) / 8.0


def test_builders_cover_what_they_promise():
    lengths = sorted(set(ar.RESIDENT_LENGTHS + ar.STREAM_LENGTHS + ar.STREAM_MAX[:1]))
    for n in lengths:
        if n >= 2:   # key n-1 carries between 0.2 and 0.8 of the mass for at least a quarter of the queries
            p = torch.softmax(_scaled_logits(ar.build("last_key", B, n, H), n), dim=-1)[..., n - 1]
            frac = float(((p > 0.2) & (p < 0.8)).double().mean())
            assert frac >= 0.25, (n, frac)
        if n >= 32:
            p = torch.softmax(_scaled_logits(ar.build("peaked", B, n, H), n), dim=-1)
            top = p.max(-1).values
            assert float(top.median()) > 0.9, (n, float(top.median()))
            assert float(((top > 0.3) & (top < 0.7)).double().mean()) > 0.02, n       # and near ties do occur
        s = _scaled_logits(ar.build("offset", B, n, H), n)
        assert float(s.abs().max(-1).values.min()) > 150.0, n
        assert bool((s[:, 0::2] > 150).all()) and (H < 2 or bool((s[:, 1::2] < -150).all())), n   # both signs, by head
    for n in (129, 320, 1024, 1088, 1089):
        nb = n // ar.BK * ar.BK                                   # whole blocks (the ragged tail block may hold a single key)
        blockmax = lambda name: _scaled_logits(ar.build(name, B, n, H), n)[..., :nb].reshape(B, H, n, -1, ar.BK).max(-1).values
        up = blockmax("ascending")
        assert bool((up[..., 1:] > up[..., :-1]).all()), n        # the running maximum rises in every block, for every query
        down = blockmax("descending")
        assert bool((down[..., 1:] < down[..., :1]).all()), n     # ... or is fixed by the first block


def _fails(defect, name, n, **kw):
    qkv = ar.build(name, B, n, H)
    ref, bound, p, p_bound = ar.bounds(qkv, B, n, H, causal=kw.get("causal", False), streaming=kw.get("streaming", False))
    out, tap = ar.emulate(qkv, B, n, H, defect=defect, **kw)
    try:
        ar.assert_within(out, ref, bound, f"defect {defect} {name} {n}")
        if tap is not None:
            ncon = kw["ncon"]
            ar.assert_within(tap, ar.tapped(p, ncon), ar.tapped(p_bound, ncon), f"defect {defect} {name} {n} tap")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("streaming", [False, True])
def test_deliberate_defects_breach_the_bound(streaming):
    """Every defect fails ar.assert_within, at every length of its list where the defect can exist."""
    for n in (2, 17, 65, 288):
        assert _fails("drop_last", "last_key", n, streaming=streaming), n
        assert _fails("dup_last", "last_key", n, streaming=streaming), n
        assert _fails("drop_last", "benign", n, streaming=streaming), n
    for ncon, n in ((4, 6), (4, 201), (64, 288)):
        assert _fails("tap_shift", "benign", n, streaming=streaming, ncon=ncon), (ncon, n)
    if not streaming:
        for name in ar.CAUSAL_BUILDERS:
            for n in (2, 17, 77, 288):
                assert _fails("causal_plus", name, n, causal=True), (name, n)
                assert _fails("causal_minus", name, n, causal=True), (name, n)
    # and without a defect the same calls pass
    assert not _fails(None, "last_key", 65, streaming=streaming)
    assert not _fails(None, "benign", 201, streaming=streaming, ncon=4)
