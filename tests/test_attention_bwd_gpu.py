"""GPU: the two attention backward kernels -- LDS-resident (attention_bwd.hip, every key-block instance KB = 1 .. 9) and streaming
(attention_bwd_stream_kernel in attention_stream.hip) -- each by itself against the fp64 closed form on the same bf16 inputs, every
element of dq, dk and dv within the bound DERIVED in tests/attention_bwd_ref.py (nothing tuned to a measured error).  qkv: benign,
peaked softmax, +-200 common logit offset, a last key that carries real mass, and for the streaming kernel a running maximum that rises
in every block / is fixed by the first.  dO: benign, a single non-zero row per image, per-row magnitudes 2^-6 .. 2^6.  dpext: benign,
and +-1024 at the four corners of the concept block, with the concept block starting on, just before and just after a 16-row tile edge.
tests/test_attention_bwd_ref_cpu.py shows on the CPU that the bounds are sound and that each deliberate defect breaches them.

Every launch: dqkv lies between two blocks of 32 sentinel (NaN) rows that must stay untouched, and starts as the sentinel itself;
qkv, dO and dpext are each followed by NaN inside the same allocation (the kernels clamp their reads to the last valid row: finite
results show that they did); a second identical launch must give identical bytes.  Every case prints its worst error / bound ratios (-s)."""
import pytest
import torch

import attention_bwd_ref as br

pytestmark = pytest.mark.gpu

B, H = br.B_TEST, br.H_TEST
D = H * 64
BY_LENGTH, RESIDENT, STREAM = 0, 1, 2
SENTINEL = 0x7FC1                       # a bf16 NaN bit pattern no kernel produces
GUARD = 32
_worst = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import _lib
    return _lib.load()


def _counts(lib):
    return [int(lib.ch_debug_attention_dispatch_count(i)) for i in (2, 3)]     # resident backward, streaming backward


def _padded(x, dev, tail):
    """x (2-D or flat) followed by `tail` rows / elements of NaN in one allocation, on the device"""
    buf = torch.full((x.shape[0] + tail,) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype)
    buf[:x.shape[0]] = x
    return buf.to(dev)


def _launch(lib, qkv, dO, ext, n, ncon, kernel):
    from concepthash_amd import _lib
    rows = B * n
    out = torch.full((rows + 2 * GUARD, 3 * D), SENTINEL, dtype=torch.int16, device=qkv.device)
    rc = lib.ch_debug_attention_bwd_ex(_lib.ptr(qkv), _lib.ptr(dO), B, n, H, _lib.ptr(out[GUARD:]), _lib.ptr(ext), ncon if ext is not None else 0,
                                       kernel, _lib.stream_ptr())
    torch.cuda.synchronize()
    _lib.check(rc, "ch_debug_attention_bwd_ex")
    assert bool((out[:GUARD] == SENTINEL).all()) and bool((out[GUARD + rows:] == SENTINEL).all()), "rows around dqkv were written"
    return out[GUARD:GUARD + rows].view(torch.bfloat16)


def _case(lib, dev, group, kernel, name, do_name, n, ncon=0, ext_name=None, expect=None):
    """one launch (and its repeat) of `kernel` held to the fp64 reference, which is computed here, on the device, from the padded buffers"""
    streaming = kernel == STREAM or (kernel == BY_LENGTH and n > 288)
    qkv = _padded(br.build(name, B, n, H), dev, 64)
    dO = _padded(br.build_do(do_name, B, n, H), dev, 64)
    ext = ext4 = None
    if ext_name:
        ext = _padded(br.build_ext(ext_name, B, n, H, ncon).reshape(-1), dev, 4096)
        ext4 = ext[:B * H * ncon * (n - ncon - 1)].view(B, H, ncon, n - ncon - 1)
    ref, bound = br.bounds(qkv, dO, ext4, B, n, H, ncon=ncon, streaming=streaming)
    c0 = _counts(lib)
    got = _launch(lib, qkv, dO, ext, n, ncon, kernel)
    c1 = _counts(lib)
    want = [0, 1] if (expect if expect is not None else kernel) == STREAM else [1, 0]
    assert [c1[0] - c0[0], c1[1] - c0[1]] == want, f"the {'streaming' if want[1] else 'resident'} backward kernel did not run"
    what = f"{group} {name} dO {do_name} ext {ext_name} {n} tokens ncon {ncon}"
    r = br.assert_all_within(got, ref, bound, what)
    _worst[group] = tuple(max(a, b) for a, b in zip(_worst.get(group, (0.0, 0.0, 0.0)), r))
    again = _launch(lib, qkv, dO, ext, n, ncon, kernel)
    assert torch.equal(again.view(torch.int16), got.view(torch.int16)), what + ": a second launch gave other bytes"
    if n == 1:   # one key: P = 1 and dV = dO, bit for bit (dq and dk are 0 up to the bound: a fused s * c - mxs leaves exp2(residual) != 1)
        assert torch.equal(got[:, 2 * D:].view(torch.int16), dO[:B].view(torch.int16))
    return got


def _report(group):
    w = _worst[group]
    print(f"WORST {group}: dq {w[0]:.3f} dk {w[1]:.3f} dv {w[2]:.3f}")


@pytest.mark.parametrize("name", br.BUILDERS)
def test_resident_kernel_within_the_derived_bound(dev, lib, name):
    group = f"resident {name}"
    for n in br.RESIDENT_LENGTHS:
        for do_name in ("benign", "one_row"):
            _case(lib, dev, group, RESIDENT, name, do_name, n)
    for n in br.SCALED_LENGTHS:
        _case(lib, dev, group, RESIDENT, name, "scaled", n)
    _report(group)


@pytest.mark.parametrize("ncon", br.TAP_NCON)
def test_resident_kernel_with_a_cotangent_on_the_probabilities(dev, lib, ncon):
    """ncon + 2 is the smallest problem; 35, 36, 37 put the first of four concept rows at 31, 32, 33 (the wave-uniform shortcut
    `qt * 16 + 15 >= q_con0`); ncon = 15, 16, 17 do the same at 201 and 288"""
    for ext_name in br.EXT_BUILDERS:
        group = f"resident ext {ext_name}"
        for n in br.ext_lengths(ncon):
            for name in br.TAP_BUILDERS:
                _case(lib, dev, group, RESIDENT, name, "benign", n, ncon=ncon, ext_name=ext_name)
        _report(group)


def _stream_pair(lib, dev, group, name, n, ncon):
    _case(lib, dev, group, STREAM, name, "benign", n)
    if n >= ncon + 2:
        _case(lib, dev, group, STREAM, name, "benign", n, ncon=ncon, ext_name="benign")


@pytest.mark.parametrize("name", br.STREAM_BUILDERS)
def test_streaming_kernel_within_the_derived_bound(dev, lib, name):
    group = f"streaming {name}"
    for n in br.STREAM_LENGTHS:
        _stream_pair(lib, dev, group, name, n, br.STREAM_NCON)
    _stream_pair(lib, dev, group, name, *br.STREAM_MAX)
    _report(group)


@pytest.mark.parametrize("n", br.STREAM_NCON_LENGTHS)
def test_streaming_kernel_concept_block_at_tile_edges(dev, lib, n):
    group = "streaming ncon edges"
    for ncon in br.STREAM_NCON_EDGE:
        for ext_name in br.EXT_BUILDERS:
            _case(lib, dev, group, STREAM, "benign", "benign", n, ncon=ncon, ext_name=ext_name)
            _case(lib, dev, group, STREAM, "peaked", "one_row", n, ncon=ncon, ext_name=ext_name)
    _report(group)


def test_dispatch_by_length(dev, lib):
    """kernel = 0: 288 tokens reach the resident kernel, 289 the streaming one (the counters are asserted inside _case)"""
    for n, expect in ((288, RESIDENT), (289, STREAM)):
        _case(lib, dev, "by length", BY_LENGTH, "benign", "benign", n, ncon=4, ext_name="corners", expect=expect)
        _case(lib, dev, "by length", BY_LENGTH, "last_key", "one_row", n, expect=expect)
    _report("by length")
