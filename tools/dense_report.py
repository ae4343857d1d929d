#!/usr/bin/env python3
"""The rankings of the real-valued codes beside the binarised ones (profiles/search_dense.txt):
    python tools/dense_report.py [--out FILE] [--sizes cub,1m] [--metrics cosine,euclidean,dot]
Clustered SYNTHETIC codes (`concepthash_amd.synthetic.synthetic_real_codes`: class centres +-1 plus N(0, 0.78^2), both sides) -- there is
no trained checkpoint offline, so the retrieval numbers say how the rankings behave on this noise model, not on a trained head.
Per size (CUB 5,794 x 5,994 x 64; 1,024 x 1M x 64; 200 classes):
1. the ladder up to the quantisation gap: mAP@all, P@10, R@10 under the Hamming, the ternary (--margin), the asymmetric (8-bit) and
   each dense ranking, and mAP_dense - mAP_hamming;
2. per metric, timing: `dense_topk` (k = 10, prepared operands) beside `hamming_topk` and beside the torch formulation of the same
   ranking -- `torch.topk` of the [Qn, G] matrix a matmul writes -- and `evaluate_dense` (which prepares both sides) beside `evaluate`
   and `evaluate_weighted`, R = -1 and k = 1, 5, 10; and whether the scan's lists equal torch's.
One process, the variants taking turns over --rounds rounds of --calls calls each after --warmup warm-ups, HIP events
(torch.cuda.Event) around a round; the median round in microseconds per call."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"cub": (5794, 5994, 64, 200), "1m": (1024, 1_000_000, 64, 200)}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--sizes", default="cub,1m")
ap.add_argument("--metrics", default="cosine,euclidean,dot")
ap.add_argument("--margin", type=float, default=0.5)
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


def torch_topk(xq, xg, metric, k):
    """the same ranking through a [Qn, G] matrix: what the scan is an alternative to (ties and the last bits may differ)"""
    if metric == "cosine":
        D = 1.0 - torch.nn.functional.normalize(xq, dim=1) @ torch.nn.functional.normalize(xg, dim=1).T
    elif metric == "dot":
        D = -(xq @ xg.T)
    else:
        D = (xq * xq).sum(1)[:, None] + (xg * xg).sum(1)[None, :] - 2.0 * (xq @ xg.T)
    d, i = torch.topk(D, k, dim=1, largest=False)
    return i, d


def row(name, r):
    return f"  {name:24s} mAP@all {r['mAP']:.4f}  P@10 {r['precisions'][2]:.4f}  R@10 {r['recalls'][2]:.4f}"


metrics = a.metrics.split(",")
lines = [f"{torch.cuda.get_device_name(0)}; R = -1, k = {KS}; timings: median of {a.rounds} rounds of {a.calls} calls per variant, the variants "
         f"taking turns, after {a.warmup} warm-ups each; torch.cuda.Event around a round; microseconds per call",
         "codes: SYNTHETIC -- class centres +-1 plus N(0, 0.78^2) on both sides (concepthash_amd.synthetic.synthetic_real_codes); the retrieval "
         "numbers describe this noise model, not a trained head"]
for name in a.sizes.split(","):
    Qn, G, n, C = SIZES[name]
    xq, ql = synthetic_real_codes(Qn, n, seed=1, nclass=C, device="cuda")
    xg, gl = synthetic_real_codes(G, n, seed=2, nclass=C, device="cuda")
    q, g = rt.pack_sign(xq), rt.pack_sign(xg)
    lines.append("")
    lines.append(f"{name}: {Qn} x {G} x {n}, {C} classes; dense top-k segments of {rt._lib.load().ch_dense_topk_seg_rows(Qn, G)} rows")
    ham = rt.evaluate(q, g, ql, gl, R=-1, ks=KS)
    lines.append(row("hamming", ham))
    lines.append(row(f"ternary, margin {a.margin:g}", rt.evaluate_ternary(rt.pack_ternary(xq, a.margin), rt.pack_ternary(xg, a.margin), n, ql, gl,
                                                                         R=-1, ks=KS)))
    lines.append(row("asymmetric, 8-bit", rt.evaluate_weighted(xq, g, ql, gl, bits=8, R=-1, ks=KS)))
    for m in metrics:
        r = rt.evaluate_dense(xq, xg, ql, gl, m, R=-1, ks=KS)
        lines.append(row(m, r) + f"  quantisation gap {r['mAP'] - ham['mAP']:+.4f}")
    for m in metrics:
        pq, pg = rt.prepare_dense(xq, m), rt.prepare_dense(xg, m)
        idx, _ = rt.dense_topk(pq, pg, m, 10)
        tidx, _ = torch_topk(xq, xg, m, 10)
        same = float((idx == tidx).all(1).float().mean().item())
        top = medians({"hamming_topk": lambda: rt.hamming_topk(q, g, 10), "dense_topk": lambda: rt.dense_topk(pq, pg, m, 10),
                       "prepare_dense (gallery)": lambda: rt.prepare_dense(xg, m), "torch.topk(matrix)": lambda: torch_topk(xq, xg, m, 10)})
        lines.append(f"  {m}: top-k, k = 10: " + " | ".join(f"{k} {v:.1f} us" for k, v in top.items()) +
                     f" | dense_topk / torch {top['dense_topk'] / top['torch.topk(matrix)']:.2f}x, / hamming_topk "
                     f"{top['dense_topk'] / top['hamming_topk']:.2f}x; lists equal to torch's for {100 * same:.1f} % of the queries")
        ev = medians({"evaluate (hamming)": lambda: rt.evaluate(q, g, ql, gl, R=-1, ks=KS),
                      "evaluate_weighted, 8-bit": lambda: rt.evaluate_weighted(xq, g, ql, gl, bits=8, R=-1, ks=KS),
                      "evaluate_dense": lambda: rt.evaluate_dense(xq, xg, ql, gl, m, R=-1, ks=KS)})
        lines.append(f"  {m}: evaluation: " + " | ".join(f"{k} {v:.1f} us ({v / ev['evaluate (hamming)']:.2f}x)" for k, v in ev.items()))
        del pq, pg
    del xq, xg, q, g
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
