"""CPU: the host side of the attention dispatch past 288 tokens -- argument checks that return before anything is launched, the
option that forces the streaming kernels, and the limits the messages name (no GPU needed: every call below fails on the host)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import _lib, build
    build.build()
    return _lib.load()


def _attn(lib, ntok, kernel, backward=False):
    buf = (ctypes.c_char * 16)()                    # non-null, never dereferenced: the calls below are refused before any launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    if backward:
        st = lib.ch_debug_attention_bwd_ex(p, p, 1, ntok, 1, p, None, 0, kernel, None)
    else:
        st = lib.ch_debug_attention_ex(p, 1, ntok, 1, p, None, 0, 0, kernel, None)
    return st, lib.ch_last_error().decode()


@pytest.mark.parametrize("backward", [False, True])
def test_kernel_selector_and_length_limits_are_checked_on_the_host(lib, backward):
    st, msg = _attn(lib, 201, 3, backward)
    assert st != 0 and "kernel must be 0" in msg
    st, msg = _attn(lib, 289, 1, backward)           # the resident kernels exist up to 288 tokens only
    assert st != 0 and "at most 288 tokens" in msg
    for kernel in (0, 2):                            # past a 32 x 32 patch grid + 64 concept tokens nothing is built
        st, msg = _attn(lib, 1 + 32 * 32 + 64 + 1, kernel, backward)
        assert st != 0 and "32 x 32 patch grid" in msg
    assert lib.ch_debug_attention_dispatch_count(4) == -1 and lib.ch_debug_attention_dispatch_count(0) >= 0


def test_option_and_limit_are_declared():
    from concepthash_amd import _lib
    assert "attn_stream" in _lib.OPTION_KEYS and "attn_stream" not in {k for k, _ in _lib._ENV_OVERRIDES.values()}
    model = open(os.path.join(ROOT, "concepthash_amd", "csrc", "model.hip")).read()
    assert re.search(r'\{"attn_stream", 0, CH_OPT_FIELD\(attn_stream\), 0, 1\}', model)
    assert 'grid <= 32' in model and "288 tokens per image is not supported" not in model
    kernels = open(os.path.join(ROOT, "concepthash_amd", "csrc", "kernels.h")).read()
    assert "CH_ATTN_RESIDENT_MAX_TOKENS = 288" in kernels and "CH_ATTN_MAX_TOKENS = 1 + 32 * 32 + 64" in kernels
