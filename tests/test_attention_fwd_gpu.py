"""GPU: the forward attention kernels -- LDS-resident (attention.hip, every key-block instance KB = 1 .. 9), its causal instance, and
streaming (attention_stream.hip) -- each by itself against fp64 attention on the same bf16 inputs, element by element within the
bound DERIVED in tests/attention_ref.py (bf16 rounding of P and of the output, the fp32 accumulations, exp2 / reciprocal, the per-block
rescale; nothing tuned to a measured error).  Inputs: benign, peaked softmax, +-200 common logit offset, a last key that carries real
mass, and for the streaming kernel a running maximum that rises in every block / is fixed by the first.  tests/test_attention_ref_cpu.py
shows on the CPU that the bound is sound and that off-by-one defects breach it.

Every launch: `out` starts as a NaN sentinel with 32 extra rows that must stay untouched; qkv is followed by 64 rows of NaN inside the
same allocation (the kernels clamp their reads to the last valid row: a finite result shows that they did).  Every case prints its
worst error / bound ratio (-s)."""
import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

B, H = ar.B_TEST, ar.H_TEST
D = H * 64
RESIDENT, STREAM = 1, 2
SENTINEL = 0x7FC1                       # a bf16 NaN bit pattern no kernel produces
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import _lib
    return _lib.load()


def _counts(lib):
    return [int(lib.ch_debug_attention_dispatch_count(i)) for i in range(2)]


def _case(name, n, dev, causal=False, streaming=False):
    """(qkv on the device with its NaN tail, out_ref, out_bound, p, p_bound): computed once, shared, never modified"""
    key = (name, n, causal, streaming)
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        qkv = ar.build(name, B, n, H)
        buf = torch.full((B * n + 64, 3 * D), float("nan"), dtype=torch.bfloat16)
        buf[:B * n] = qkv
        buf = buf.to(dev)
        _cache[key] = (buf,) + ar.bounds(buf, B, n, H, causal=causal, streaming=streaming)
    return _cache[key]


def _launch(lib, buf, n, kernel, ncon=0, tap=False, compact=False, causal=False, expect_error=False):
    from concepthash_amd import _lib
    rows = B * (1 + ncon) if compact else B * n
    out = torch.full((rows + 32, D), SENTINEL, dtype=torch.int16, device=buf.device).view(torch.bfloat16)
    cattn = torch.full((B, H, ncon, n - ncon - 1), float("nan"), dtype=torch.float32, device=buf.device) if tap else None
    if causal:
        rc = lib.ch_debug_attention_causal(_lib.ptr(buf), B, n, H, _lib.ptr(out), _lib.stream_ptr())
    else:
        rc = lib.ch_debug_attention_ex(_lib.ptr(buf), B, n, H, _lib.ptr(out), _lib.ptr(cattn), ncon, int(compact), kernel, _lib.stream_ptr())
    torch.cuda.synchronize()
    if expect_error:
        assert rc != 0 and lib.ch_last_error(), "the launch should have been refused with a status"
        assert bool((out.view(torch.int16) == SENTINEL).all())
        return None, None
    _lib.check(rc, "attention tap")
    assert bool((out[rows:].view(torch.int16) == SENTINEL).all()), "rows past the output were written"
    return out[:rows], cattn


def _v_rows(buf, n, token):
    """v of one token of every image, as the output row layout [B, H*64]"""
    return buf[:B * n].view(B, n, 3, D)[:, token, 2]


@pytest.mark.parametrize("name", ar.BUILDERS)
def test_resident_kernel_within_the_derived_bound(dev, lib, name):
    for n in ar.RESIDENT_LENGTHS:
        buf, ref, bound, _, _ = _case(name, n, dev)
        c0 = _counts(lib)
        out, _ = _launch(lib, buf, n, RESIDENT)
        c1 = _counts(lib)
        assert c1[0] - c0[0] == 1 and c1[1] == c0[1], "the resident kernel did not run"
        ar.assert_within(out, ref, bound, f"resident {name} {n} tokens")
        if n == 1:
            assert torch.equal(out.view(torch.int16), _v_rows(buf, 1, 0).view(torch.int16))     # one key: the output is v, bit for bit


@pytest.mark.parametrize("ncon", ar.TAP_NCON)
def test_resident_tap_and_compact_mode(dev, lib, ncon):
    for name in ar.TAP_BUILDERS:
        for n in ar.tap_lengths(ncon):
            buf, ref, bound, p, p_bound = _case(name, n, dev)
            what = f"resident {name} {n} tokens ncon {ncon}"
            full, tap = _launch(lib, buf, n, RESIDENT, ncon=ncon, tap=True)
            ar.assert_within(full, ref, bound, what + " full")
            ar.assert_within(tap, ar.tapped(p, ncon), ar.tapped(p_bound, ncon), what + " tap")    # finite: every entry written
            rows = ar.head_rows(B, n, ncon).to(dev)
            for with_tap in (False, True):
                comp, ctap = _launch(lib, buf, n, RESIDENT, ncon=ncon, tap=with_tap, compact=True)
                assert torch.equal(comp.view(torch.int16), full[rows].view(torch.int16)), (what, with_tap)
                if with_tap:
                    assert torch.equal(ctap, tap), what


@pytest.mark.parametrize("name", ar.CAUSAL_BUILDERS)
def test_causal_instance_within_the_derived_bound(dev, lib, name):
    for n in ar.CAUSAL_LENGTHS:
        buf, ref, bound, _, _ = _case(name, n, dev, causal=True)
        out, _ = _launch(lib, buf, n, RESIDENT, causal=True)
        ar.assert_within(out, ref, bound, f"causal {name} {n} tokens")
        assert torch.equal(out.view(B, n, D)[:, 0].view(torch.int16), _v_rows(buf, n, 0).view(torch.int16))   # row 0 sees key 0 only


def _stream_case(dev, lib, name, n, ncon):
    buf, ref, bound, p, p_bound = _case(name, n, dev, streaming=True)
    what = f"streaming {name} {n} tokens ncon {ncon}"
    tap_on = n >= ncon + 2
    c0 = _counts(lib)
    full, tap = _launch(lib, buf, n, STREAM, ncon=ncon if tap_on else 0, tap=tap_on)
    c1 = _counts(lib)
    assert c1[1] - c0[1] == 1 and c1[0] == c0[0], "the streaming kernel did not run"
    ar.assert_within(full, ref, bound, what)
    if n == 1:
        assert torch.equal(full.view(torch.int16), _v_rows(buf, 1, 0).view(torch.int16))
    if tap_on:
        ar.assert_within(tap, ar.tapped(p, ncon), ar.tapped(p_bound, ncon), what + " tap")
        plain, _ = _launch(lib, buf, n, STREAM)
        assert torch.equal(plain.view(torch.int16), full.view(torch.int16)), what       # the tap changes nothing in the output
    if n > ncon:
        rows = ar.head_rows(B, n, ncon).to(dev)
        for with_tap in ((False, True) if tap_on else (False,)):
            comp, ctap = _launch(lib, buf, n, STREAM, ncon=ncon, tap=with_tap, compact=True)
            assert torch.equal(comp.view(torch.int16), full[rows].view(torch.int16)), (what, with_tap)
            if with_tap:
                assert torch.equal(ctap, tap), what


@pytest.mark.parametrize("name", ar.STREAM_BUILDERS)
def test_streaming_kernel_within_the_derived_bound(dev, lib, name):
    for n in ar.STREAM_LENGTHS:
        _stream_case(dev, lib, name, n, ar.STREAM_NCON)
    _stream_case(dev, lib, name, *ar.STREAM_MAX)


def test_lengths_past_the_limits_are_refused(dev, lib):
    for n, kw in ((289, dict(kernel=RESIDENT, causal=True)), (289, dict(kernel=RESIDENT)), (1090, dict(kernel=STREAM)), (1090, dict(kernel=0))):
        buf = torch.zeros(B * n + 64, 3 * D, dtype=torch.bfloat16, device=dev)
        _launch(lib, buf, n, expect_error=True, **kw)
