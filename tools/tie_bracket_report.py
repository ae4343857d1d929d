"""How much can the order of equal-distance rows move mAP?  ("tie bracket")

    python tools/tie_bracket_report.py [--out profiles/r06_tie_bracket_report.json] [--sizes cub,nabirds,1m] [--reps 3]

For seeded inputs of its own at the three evaluation sizes of bench.py's `map_eval` block it prints, and writes as JSON: the stable
mAP@all (ties by gallery index), the smallest and the largest mAP any tie order can give, the width of that bracket, the time of the
bracket kernel from HIP events and the time of the `evaluate` call it rides on (their ratio is the cost of `tie_bracket=True`).
Inputs: (a) the recipe of `map_eval` restated -- uniformly random packed codes and labels, generator seed 7; (b) clustered codes --
one random centre per class, every bit of a row flipped with probability 0.10 / 0.25: what trained codes look like, and where the
buckets next to a query are relevant-heavy.  mAP@R for R in {100, 1000} is reported beside mAP@all: a limit cuts one bucket, where
the bracket is widest.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"cub": ("CUB-200 size", 5794, 5994, 64, 200), "nabirds": ("NABirds size", 24633, 23929, 64, 555),
         "1m": ("BASELINE config 5 size", 16384, 1_000_000, 128, 200)}
RS = [100, 1000, -1]


def uniform_inputs(torch, dev, qn, gn, nbit, ncls):
    W = nbit // 64
    gen = torch.Generator(device=dev).manual_seed(7)
    q = torch.randint(-2 ** 63, 2 ** 63 - 1, (qn, W), dtype=torch.int64, device=dev, generator=gen)
    g = torch.randint(-2 ** 63, 2 ** 63 - 1, (gn, W), dtype=torch.int64, device=dev, generator=gen)
    ql = torch.randint(0, ncls, (qn,), dtype=torch.int32, device=dev, generator=gen)
    gl = torch.randint(0, ncls, (gn,), dtype=torch.int32, device=dev, generator=gen)
    return q, g, ql, gl


def clustered_inputs(torch, rt, dev, qn, gn, nbit, ncls, flip):
    gen = torch.Generator(device=dev).manual_seed(7)
    centres = torch.randint(0, 2, (ncls, nbit), device=dev, generator=gen, dtype=torch.int8)

    def rows(n):
        lab = torch.randint(0, ncls, (n,), dtype=torch.int32, device=dev, generator=gen)
        out = torch.empty(n, nbit // 64, dtype=torch.int64, device=dev)
        for r0 in range(0, n, 1 << 18):          # blocks: the fp32 form of 1M x 128 bits is 512 MB
            lb = lab[r0:r0 + (1 << 18)].long()
            noise = torch.rand(lb.shape[0], nbit, device=dev, generator=gen) < flip
            bits = centres[lb].bool() ^ noise
            out[r0:r0 + lb.shape[0]] = rt.pack_sign(bits.float() * 2 - 1)
        return out, lab
    q, ql = rows(qn)
    g, gl = rows(gn)
    return q, g, ql, gl


def event_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    return best


def report(torch, rt, name, q, g, ql, gl, reps):
    ev = rt.evaluate(q, g, ql, gl, R=RS, ks=(1, 5, 10), tie_bracket=True)
    W = q.shape[1]
    seg = rt.map_seg_rows(q.shape[0], g.shape[0], W)
    counts = rt.hamming_hist(q, g, ql, gl, 0, seg).sum(0, dtype=torch.int32)
    limits, _ = rt.normalize_limits(RS)
    k_ms = event_ms(torch, lambda: rt.tie_bracket(counts, limits), reps)
    k_all_ms = event_ms(torch, lambda: rt.tie_bracket(counts, [0]), reps)
    e_ms = event_ms(torch, lambda: rt.evaluate(q, g, ql, gl, R=RS, ks=(1, 5, 10)), reps)
    e_tie_ms = event_ms(torch, lambda: rt.evaluate(q, g, ql, gl, R=RS, ks=(1, 5, 10), tie_bracket=True), reps)
    nz = counts[..., 0] > 0
    row = {"inputs": name, "evaluate_ms": round(e_ms, 3), "evaluate_tie_bracket_ms": round(e_tie_ms, 3),
           "tie_kernel_ms": round(k_ms, 3), "tie_kernel_over_evaluate": round(k_ms / e_ms, 4), "tie_kernel_mAP_all_only_ms": round(k_all_ms, 3),
           "nonempty_buckets_per_query": round(float(nz.sum(1).double().mean()), 2),
           "deepest_bucket_rows": int(counts[..., 0].max()), "deepest_bucket_relevant_rows": int(counts[..., 1].max())}
    for i, R in enumerate(RS):
        tag = "all" if R <= 0 else str(R)
        lo, hi = ev["mAP_low"][i], ev["mAP_high"][i]
        row["mAP@" + tag] = {"stable": ev["mAP"][i], "low": lo, "high": hi, "width": hi - lo, "holds_1e-3_for_any_tie_order": bool(hi - lo < 1e-3)}
        print(f"  {name:<24} mAP@{tag:<5} {ev['mAP'][i]:.6f}  [{lo:.6f}, {hi:.6f}]  width {hi - lo:.3e}")
    print(f"  {name:<24} bracket kernel {k_ms:.3f} ms ({k_all_ms:.3f} ms for mAP@all alone), evaluate {e_ms:.3f} ms -> {e_tie_ms:.3f} ms with the switch")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_tie_bracket_report.json"))
    ap.add_argument("--sizes", default="cub,nabirds,1m")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from concepthash_amd import retrieval as rt
    if not torch.cuda.is_available():
        raise SystemExit("tie_bracket_report needs the GPU")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "R": RS, "sizes": {}}
    for key in a.sizes.split(","):
        label, qn, gn, nbit, ncls = SIZES[key]
        print(f"{label}: {qn} queries x {gn} gallery rows x {nbit} bit, {ncls} classes")
        rows = [report(torch, rt, "uniform (seed 7)", *uniform_inputs(torch, dev, qn, gn, nbit, ncls), a.reps)]
        for flip in (0.10, 0.25):
            rows.append(report(torch, rt, f"clustered, flip {flip:.2f}", *clustered_inputs(torch, rt, dev, qn, gn, nbit, ncls, flip), a.reps))
        out["sizes"][key] = {"workload": f"{label}: {qn} x {gn} x {nbit} bit, {ncls} classes", "inputs": rows}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:          # after every size: a long run leaves what it has
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
