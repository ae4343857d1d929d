"""The launch discipline that the single-kernel GPU tests share (tests/test_train_rowkernels_gpu.py, tests/test_forward_kernels_gpu.py,
tests/test_gemm_fwd_epilogues_gpu.py; tests/test_gemm_train_epilogues_gpu.py takes its sentinel buffers from here):
each output lies between two guard blocks of a sentinel (a NaN bit pattern no kernel produces) that must come back untouched, and starts as
the sentinel itself, so an element the kernel failed to write is seen; every input is followed by NaN inside the same allocation; a second
identical launch must give identical bytes; the worst error / bound ratio of every group of comparisons is kept and printed."""
import ctypes

import torch

from train_kernels_ref import assert_within

SENT32 = 0x7FC1BEEF                      # fp32 / bf16 NaN bit patterns no kernel produces
SENT16 = 0x7FC1
SENT64 = 0x7FC1BEEF7FC1BEEF              # the same for 64-bit words (packed codes)
GUARD = 64                               # elements on either side of an output
TAIL = 64                                # NaN elements behind an input
_worst = {}
_ITEM = {torch.float32: (torch.int32, SENT32), torch.bfloat16: (torch.int16, SENT16), torch.int64: (torch.int64, SENT64)}


class Out:
    """an output of `shape` (fp32, bf16 or 64-bit words) between guards, all of it the sentinel; `init` (in / out operands) replaces the
    payload"""

    def __init__(self, dev, shape, dtype, init=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.it, self.sent = _ITEM[dtype]
        self.buf = torch.full((self.n + 2 * GUARD,), self.sent, dtype=self.it, device=dev)
        if init is not None:
            self.buf[GUARD:GUARD + self.n] = init.contiguous().view(self.it).reshape(-1).to(dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def raw(self):
        """the payload's bits on the CPU, after checking the guards"""
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.sent).all()) and bool((b[GUARD + self.n:] == self.sent).all()), "a guard block was written"
        return b[GUARD:GUARD + self.n].view(self.shape)

    def get(self):
        return self.raw().view(self.dtype)

    def untouched(self, mask):
        """True when every payload element under `mask` (CPU bool tensor of the payload's shape) is still the sentinel"""
        return bool((self.raw()[mask] == self.sent).all())


def sentinel(rows, ld):
    """a [rows, ld] bf16 buffer (as int16) on the GPU, all of it SENT16"""
    return torch.full((rows, ld), SENT16, dtype=torch.int16, device="cuda")


def untouched(buf, M, N):
    """rows >= M and the gap columns >= N of a sentinel-filled [rows, ld] bf16 buffer"""
    return bool((buf[M:] == SENT16).all()) and bool((buf[:M, N:] == SENT16).all())


def inp(dev, x):
    """x on the device, followed by TAIL NaN elements in the same allocation (returns the view of x; the base stays alive through it)"""
    buf = torch.full((x.numel() + TAIL,), float("nan"), dtype=x.dtype)
    buf[:x.numel()] = x.reshape(-1)
    return buf.to(dev)[:x.numel()].view(x.shape)


def twice(launch):
    """launch() -> list of Out, run two times on fresh outputs: returns the first run's, asserts the second's bytes are the same"""
    a = launch()
    torch.cuda.synchronize()
    b = launch()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.raw(), y.raw()), "a second identical launch gave other bytes"
    return a


def note(group, ratio):
    _worst[group] = max(_worst.get(group, 0.0), ratio)


def report(*groups):
    for g in groups:
        print(f"WORST {g}: {_worst.get(g, 0.0):.3f}")


def within(group, got, ref, bound, what):
    note(group, assert_within(got, ref, bound, f"{group} {what}", quiet=True))
