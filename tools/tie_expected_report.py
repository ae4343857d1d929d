"""Where inside the tie bracket does mAP lie on average?  ("tie expectation")

    python tools/tie_expected_report.py [--out profiles/tie_expected_report.json] [--sizes cub,nabirds,1m] [--reps 3]

For seeded synthetic inputs at the CUB-200, NABirds and 1,024 x 1M sizes -- the uniform and the clustered codes of
tools/tie_bracket_report.py -- at 64 bits and for ONE 16-bit sub-code (the first concept's columns: 17 distances, where ties weigh
most), it prints and writes as JSON: the stable mAP (ties by gallery index), the expected mAP over every tie order, the bracket, and
expected - stable; the time of the expectation kernel from HIP events beside the bracket kernel's on the same counts and beside the
`evaluate` call both ride on.  No time is promised: what is recorded is the ratio to the bracket kernel, on the device named in the file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from tie_bracket_report import clustered_inputs, event_ms, uniform_inputs  # noqa: E402

SIZES = {"cub": ("CUB-200 size", 5794, 5994, 64, 200), "nabirds": ("NABirds size", 24633, 23929, 64, 555),
         "1m": ("1,024 x 1M size", 1024, 1_000_000, 64, 200)}
RS = [100, 1000, -1]
KS = (1, 5, 10)
SUB_BITS = 16


def report(torch, rt, name, q, g, ql, gl, reps):
    ev = rt.evaluate(q, g, ql, gl, R=RS, ks=KS, tie_bracket=True, tie_expected=True)
    seg = rt.map_seg_rows(q.shape[0], g.shape[0], q.shape[1])
    counts = rt.hamming_hist(q, g, ql, gl, 0, seg).sum(0, dtype=torch.int32)
    limits, _ = rt.normalize_limits(RS)
    x_ms = event_ms(torch, lambda: rt.tie_expected(counts, limits, KS), reps)
    x_all_ms = event_ms(torch, lambda: rt.tie_expected(counts, [0]), reps)
    b_ms = event_ms(torch, lambda: rt.tie_bracket(counts, limits), reps)
    e_ms = event_ms(torch, lambda: rt.evaluate(q, g, ql, gl, R=RS, ks=KS), reps)
    e_x_ms = event_ms(torch, lambda: rt.evaluate(q, g, ql, gl, R=RS, ks=KS, tie_expected=True), reps)
    row = {"inputs": name, "evaluate_ms": round(e_ms, 3), "evaluate_tie_expected_ms": round(e_x_ms, 3),
           "expected_kernel_ms": round(x_ms, 3), "expected_kernel_mAP_all_only_ms": round(x_all_ms, 3), "bracket_kernel_ms": round(b_ms, 3),
           "expected_over_bracket_kernel": round(x_ms / b_ms, 3), "expected_kernel_over_evaluate": round(x_ms / e_ms, 4),
           "deepest_bucket_rows": int(counts[..., 0].max()), "deepest_bucket_relevant_rows": int(counts[..., 1].max())}
    for i, R in enumerate(RS):
        tag = "all" if R <= 0 else str(R)
        st, ex, lo, hi = ev["mAP"][i], ev["mAP_expected"][i], ev["mAP_low"][i], ev["mAP_high"][i]
        row["mAP@" + tag] = {"stable": st, "expected": ex, "low": lo, "high": hi, "expected_minus_stable": ex - st}
        print(f"  {name:<32} mAP@{tag:<5} stable {st:.6f}  expected {ex:.6f}  [{lo:.6f}, {hi:.6f}]  expected - stable {ex - st:+.3e}")
    print(f"  {name:<32} expectation kernel {x_ms:.3f} ms ({x_all_ms:.3f} ms for mAP@all alone), bracket kernel {b_ms:.3f} ms, "
          f"evaluate {e_ms:.3f} ms -> {e_x_ms:.3f} ms with the switch")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tie_expected_report.json"))
    ap.add_argument("--sizes", default="cub,nabirds,1m")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from concepthash_amd import retrieval as rt
    if not torch.cuda.is_available():
        raise SystemExit("tie_expected_report needs the GPU")
    dev = torch.device("cuda:0")
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    out = {"measured_on": f"one {torch.cuda.get_device_name(0)} ({arch})", "R": RS, "ks": list(KS), "sub_code_bits": SUB_BITS, "sizes": {}}
    sub = torch.tensor([(1 << SUB_BITS) - 1], dtype=torch.int64, device=dev)
    for key in a.sizes.split(","):
        label, qn, gn, nbit, ncls = SIZES[key]
        print(f"{label}: {qn} queries x {gn} gallery rows x {nbit} bit, {ncls} classes")
        rows = []
        inputs = [("uniform (seed 7)", uniform_inputs(torch, dev, qn, gn, nbit, ncls))]
        inputs += [(f"clustered, flip {flip:.2f}", clustered_inputs(torch, rt, dev, qn, gn, nbit, ncls, flip)) for flip in (0.10, 0.25)]
        for name, (q, g, ql, gl) in inputs:
            rows.append(report(torch, rt, f"{name}, {nbit} bit", q, g, ql, gl, a.reps))
            rows.append(report(torch, rt, f"{name}, {SUB_BITS}-bit sub-code", q[:, :1] & sub, g[:, :1] & sub, ql, gl, a.reps))
        out["sizes"][key] = {"workload": f"{label}: {qn} x {gn} x {nbit} bit, {ncls} classes", "inputs": rows}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:          # after every size: a long run leaves what it has
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
