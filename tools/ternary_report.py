#!/usr/bin/env python3
"""Ternary codes beside the binary ones (profiles/search_ternary.txt):
    python tools/ternary_report.py [--out FILE] [--sizes cub,1m] [--margins 0,0.25,0.5,0.75,1.0]
Clustered SYNTHETIC codes (`concepthash_amd.synthetic.synthetic_real_codes`: class centres +-1 plus N(0, 0.78^2), both sides) -- there is
no trained checkpoint offline, so the retrieval numbers say how the rankings behave on this noise model, not on a trained head.
Per size (CUB 5,794 x 5,994 x 64 bit; 1,024 x 1M x 128 bit; 200 classes):
1. per margin: the share of ternary zeros (database, queries) and mAP@all, P@10, R@10 under the Hamming and the ternary ranking;
2. timing at --time-margin: `ternary_topk` beside `hamming_topk` at k = 10, and `evaluate_ternary` beside `evaluate` and
   `evaluate_weighted` (8-bit), R = -1 and k = 1, 5, 10.  One process, the variants taking turns over --rounds rounds of --calls calls
   each after --warmup warm-ups, HIP events (torch.cuda.Event) around a round; the median round in microseconds per call."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"cub": (5794, 5994, 64, 200), "1m": (1024, 1_000_000, 128, 200)}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--sizes", default="cub,1m")
ap.add_argument("--margins", default="0,0.25,0.5,0.75,1.0")
ap.add_argument("--time-margin", type=float, default=0.5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()

import torch  # noqa: E402

from concepthash_amd import retrieval as rt  # noqa: E402
from concepthash_amd.synthetic import synthetic_real_codes  # noqa: E402

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


def row(name, r):
    return f"  {name:24s} mAP@all {r['mAP']:.4f}  P@10 {r['precisions'][2]:.4f}  R@10 {r['recalls'][2]:.4f}"


lines = [f"{torch.cuda.get_device_name(0)}; R = -1, k = {KS}; timings: median of {a.rounds} rounds of {a.calls} calls per variant, the variants "
         f"taking turns, after {a.warmup} warm-ups each; torch.cuda.Event around a round; microseconds per call",
         "codes: SYNTHETIC -- class centres +-1 plus N(0, 0.78^2) on both sides (concepthash_amd.synthetic.synthetic_real_codes); the retrieval "
         "numbers describe this noise model, not a trained head"]
for name in a.sizes.split(","):
    Qn, G, nbit, C = SIZES[name]
    xq, ql = synthetic_real_codes(Qn, nbit, seed=1, nclass=C, device="cuda")
    xg, gl = synthetic_real_codes(G, nbit, seed=2, nclass=C, device="cuda")
    q, g = rt.pack_sign(xq), rt.pack_sign(xg)
    lines.append("")
    lines.append(f"{name}: {Qn} x {G} x {nbit} bit, {C} classes")
    lines.append(row("hamming", rt.evaluate(q, g, ql, gl, R=-1, ks=KS)))
    for m in (float(s) for s in a.margins.split(",")):
        q3, g3 = rt.pack_ternary(xq, m), rt.pack_ternary(xg, m)
        zg, zq = 1.0 - (xg.abs() > m).float().mean().item(), 1.0 - (xq.abs() > m).float().mean().item()
        lines.append(row(f"ternary, margin {m:g}", rt.evaluate_ternary(q3, g3, nbit, ql, gl, R=-1, ks=KS)) +
                     f"  zeros: database {100 * zg:.1f} %, queries {100 * zq:.1f} %")
    m = a.time_margin
    q3, g3 = rt.pack_ternary(xq, m), rt.pack_ternary(xg, m)
    top = medians({"hamming_topk": lambda: rt.hamming_topk(q, g, 10), "ternary_topk": lambda: rt.ternary_topk(q3, g3, nbit, 10)})
    lines.append(f"  top-k, k = 10, margin {m:g}: " + " | ".join(f"{n} {v:.1f} us ({v / top['hamming_topk']:.2f}x)" for n, v in top.items()))
    ev = medians({"evaluate (hamming)": lambda: rt.evaluate(q, g, ql, gl, R=-1, ks=KS),
                  "evaluate_weighted, 8-bit": lambda: rt.evaluate_weighted(xq, g, ql, gl, bits=8, R=-1, ks=KS),
                  "evaluate_ternary": lambda: rt.evaluate_ternary(q3, g3, nbit, ql, gl, R=-1, ks=KS)})
    lines.append(f"  evaluation, margin {m:g}: " + " | ".join(f"{n} {v:.1f} us ({v / ev['evaluate (hamming)']:.2f}x)" for n, v in ev.items()))
    del xq, xg, q3, g3, q, g
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
