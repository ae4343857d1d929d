#!/usr/bin/env python3
"""Masked against unmasked top-k (profiles/search_masked_topk.txt):
    python tools/masked_topk_bench.py [--out FILE]
hamming_topk, hamming_topk_masked with one shared mask and with per-query masks, k = 10, at 5,794 x 5,994 x 64 bit and
16,384 x 1M x 128 bit; torch.cuda.Event around 20 calls after 5 warm-ups; microseconds per call and the masked / unmasked ratios."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from concepthash_amd import retrieval as rt

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
a = ap.parse_args()
gen = torch.Generator(device="cuda").manual_seed(1234)


def rand(rows, W):
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (rows, W), dtype=torch.int64, device="cuda", generator=gen)


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.calls          # microseconds per call


lines = [f"{torch.cuda.get_device_name(0)}; k = 10; {a.calls} calls after {a.warmup} warm-ups, torch.cuda.Event around the calls"]
for Qn, G, nbit in ((5794, 5994, 64), (16384, 1_000_000, 128)):
    W = nbit // 64
    q, g, per_query = rand(Qn, W), rand(G, W), rand(Qn, W)
    shared = per_query[0].clone()
    plain = timed(lambda: rt.hamming_topk(q, g, 10))
    one = timed(lambda: rt.hamming_topk_masked(q, g, shared, 10))
    each = timed(lambda: rt.hamming_topk_masked(q, g, per_query, 10))
    lines.append(f"{Qn} x {G} x {nbit} bit: hamming_topk {plain:10.1f} us | masked, shared mask {one:10.1f} us ({one / plain:.3f}x) | "
                 f"masked, per-query masks {each:10.1f} us ({each / plain:.3f}x)")
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
