#!/usr/bin/env python3
"""Micro-benchmark + fp32 check of the attention kernels, forward and backward.
python tools/attn_bench.py [--batch 256] [--ntok 201 288 581 789] [--heads 12] [--kernel auto resident stream] [--backward]

--kernel: auto = the dispatch rule (up to 288 tokens the LDS-resident kernel, past them the streaming one), resident / stream force
one (resident exists up to 288 tokens only).  Several --ntok / --kernel values give one line per combination."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from concepthash_amd import _lib

KERNELS = {"auto": 0, "resident": 1, "stream": 2}
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--ntok", type=int, nargs="+", default=[201])
ap.add_argument("--heads", type=int, default=12)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--kernel", nargs="+", choices=sorted(KERNELS), default=["auto"])
ap.add_argument("--backward", action="store_true", help="also time ch_attention_bwd (2.5x the forward's FLOPs, reads qkv + dO, writes dqkv)")
a = ap.parse_args()
lib = _lib.load()
B, H = a.batch, a.heads
D = H * 64


def timed(fn):
    ts = []
    for r in range(a.rounds + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


for N in a.ntok:
    qkv = torch.randn(B * N, 3 * D, device="cuda").to(torch.bfloat16)
    out = torch.empty(B * N, D, dtype=torch.bfloat16, device="cuda")
    dO = torch.randn(B * N, D, device="cuda").to(torch.bfloat16)
    dqkv = torch.empty(B * N, 3 * D, dtype=torch.bfloat16, device="cuda")
    nb = min(B, 2)
    q, k, v = qkv[: nb * N].float().view(nb, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).permute(0, 2, 1, 3).reshape(nb * N, D)
    for name in a.kernel:
        if name == "resident" and N > 288:
            continue
        kern = KERNELS[name]
        used = "stream" if kern == 2 or (kern == 0 and N > 288) else "resident"
        med, mn = timed(lambda: _lib.check(lib.ch_debug_attention_ex(_lib.ptr(qkv), B, N, H, _lib.ptr(out), None, 0, 0, kern, _lib.stream_ptr()), "attn"))
        fl = 4.0 * B * N * N * D
        by = (B * N * 3 * D + B * N * D) * 2
        err = float((out[: nb * N].float() - ref).abs().max())
        print(f"attention forward  B={B} N={N} H={H} kernel={used}: med {med*1e3:.1f} us  {fl/med/1e9:.1f} TF  {by/med/1e6:.0f} GB/s "
              f"(min {mn*1e3:.1f} us)  max abs err vs fp32 {err:.2e}")
        if a.backward:
            med, mn = timed(lambda: _lib.check(lib.ch_debug_attention_bwd_ex(_lib.ptr(qkv), _lib.ptr(dO), B, N, H, _lib.ptr(dqkv), None, 0, kern,
                                                                             _lib.stream_ptr()), "attn bwd"))
            fl = 10.0 * B * N * N * D
            by = (B * N * 3 * D * 2 + B * N * D) * 2
            print(f"attention backward B={B} N={N} H={H} kernel={used}: med {med*1e3:.1f} us  {fl/med/1e9:.1f} TF  {by/med/1e6:.0f} GB/s "
                  f"(min {mn*1e3:.1f} us)")
