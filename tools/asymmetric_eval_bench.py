#!/usr/bin/env python3
"""Evaluation under the asymmetric (weighted) ranking beside the Hamming one (profiles/eval_asymmetric.txt):
    python tools/asymmetric_eval_bench.py [--out FILE] [--sizes cub,nabirds,1m]
Clustered synthetic codes: class centres +-1, query code = centre + N(0, 0.78^2) (about 10 % sign flips), gallery = sign of the same
model.  Per size (CUB 5,794 x 5,994 x 64 bit, 200 classes; NABirds 24,633 x 23,929 x 64 bit, 555 classes; 1,024 x 1M x 128 bit, 200
classes):
1. Timing: `retrieval.evaluate` and `retrieval.evaluate_weighted` with 4-bit and 8-bit weights on the same codes, R = -1 and
   k = 1, 5, 10; one process, the variants taking turns over --rounds rounds of --calls calls each after --warmup warm-ups (the
   protocol of tools/weighted_topk_bench.py: torch.cuda.Event around a round); the median round in microseconds per call.
2. Where the time of evaluate_weighted goes: collect (count, prefix, write) / sort / scan / AP from bins, each step alone under the same
   protocol (8-bit weights), as shares of their sum.
3. mAP@all, P@10 and R@10 under the Hamming ranking and under both weighted ones."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"cub": (5794, 5994, 64, 200), "nabirds": (24633, 23929, 64, 555), "1m": (1024, 1_000_000, 128, 200)}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--sizes", default="cub,nabirds,1m")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()

import torch  # noqa: E402

from concepthash_amd import retrieval as rt  # noqa: E402

gen = torch.Generator(device="cuda").manual_seed(1234)
KS = (1, 5, 10)


def round_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.calls


def medians(variants):
    """the variants taking turns -> {name: median round, us per call}"""
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(a.rounds):
        for n, fn in variants.items():
            times[n].append(round_us(fn))
    return {n: statistics.median(v) for n, v in times.items()}


lines = [f"{torch.cuda.get_device_name(0)}; R = -1, k = {KS}; median of {a.rounds} rounds of {a.calls} calls per variant, the variants taking "
         f"turns, after {a.warmup} warm-ups each; torch.cuda.Event around a round; microseconds per call",
         "codes: class centres +-1, query = centre + N(0, 0.78^2), gallery = sign(centre + N(0, 0.78^2))"]
for name in a.sizes.split(","):
    Qn, G, nbit, C = SIZES[name]
    centres = torch.sign(torch.randn(C, nbit, device="cuda", generator=gen))
    ql = torch.randint(0, C, (Qn,), device="cuda", generator=gen)
    gl = torch.randint(0, C, (G,), device="cuda", generator=gen)
    codes = centres[ql] + 0.78 * torch.randn(Qn, nbit, device="cuda", generator=gen)
    g = rt.pack_sign(centres[gl] + 0.78 * torch.randn(G, nbit, device="cuda", generator=gen))
    q = rt.pack_sign(codes)
    flips = (torch.sign(codes) != centres[ql]).float().mean().item()
    res = {"hamming": rt.evaluate(q, g, ql, gl, R=-1, ks=KS)}
    for bits in (4, 8):
        res[f"weighted, {bits}-bit"] = rt.evaluate_weighted(codes, g, ql, gl, bits=bits, R=-1, ks=KS)
    med = medians({"evaluate (hamming)": lambda: rt.evaluate(q, g, ql, gl, R=-1, ks=KS),
                   "evaluate_weighted, 4-bit": lambda: rt.evaluate_weighted(codes, g, ql, gl, bits=4, R=-1, ks=KS),
                   "evaluate_weighted, 8-bit": lambda: rt.evaluate_weighted(codes, g, ql, gl, bits=8, R=-1, ks=KS)})
    lines.append("")
    lines.append(f"{name}: {Qn} x {G} x {nbit} bit, {C} classes, {100 * flips:.1f} % of the query signs differ from the centre's")
    lines.append("  " + " | ".join(f"{n} {v:10.1f} us ({v / med['evaluate (hamming)']:.2f}x)" for n, v in med.items()))
    # the steps of evaluate_weighted, 8-bit weights
    planes, _ = rt.weight_planes(codes, 8)
    q_lab, g_lab, LW = rt.prepare_labels(ql, gl)
    offsets, keys, longest = rt.rank_collect(q, planes, g, q_lab, g_lab, LW)
    skeys = rt.sort_slices(offsets, keys)
    cap = max(1, min(rt.RANK_LIST_MAX, longest))
    bins = rt.rank_count(q, planes, g, offsets, skeys, cap)
    limits, _ = rt.normalize_limits([-1] + list(KS))
    steps = medians({"pack + planes": lambda: (rt.pack_sign(codes), rt.weight_planes(codes, 8)),
                     "collect": lambda: rt.rank_collect(q, planes, g, q_lab, g_lab, LW),
                     "sort": lambda: rt.sort_slices(offsets, keys),
                     "scan": lambda: rt.rank_count(q, planes, g, offsets, skeys, cap),
                     "AP from bins": lambda: rt.rank_ap(offsets, bins, limits)})
    tot = sum(steps.values())
    lines.append(f"  steps (8-bit; {keys.numel()} relevant keys, longest list {longest}, {-(-G // rt.rank_seg_rows(Qn, G))} scan segment(s)): " +
                 " | ".join(f"{n} {v:.1f} us ({100 * v / tot:.0f} %)" for n, v in steps.items()))
    for n, r in res.items():
        lines.append(f"  {n:16s} mAP@all {r['mAP']:.4f}  P@10 {r['precisions'][2]:.4f}  R@10 {r['recalls'][2]:.4f}")
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
