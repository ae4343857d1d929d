#!/usr/bin/env python3
"""Ranked lists of any depth and radius search against the top-k scan (profiles/search_ranked_lists.txt):
    python tools/ranked_list_bench.py [--out FILE] [--parent-lib PATH/libconcepthash_hip.so]
Sizes 5,794 x 5,994 x 64 bit and 16,384 x 1M x 128 bit on clustered codes (200 class centres, codes = centre * 0.8 + N(0, 0.6), as
tools/weighted_topk_bench.py), k = 10.
1. New paths, one process, the variants taking turns over --rounds rounds of --calls calls each, 400 times as many at the small size
   (torch.cuda.Event around a round's calls, warm-ups excluded; the median round in microseconds per call): hamming_topk (k = 10 and
   128), hamming_ranked at k = 128 and k = 1000, hamming_radius at the radius that keeps a few hundred rows per query, the histogram
   pass alone, and the scatter pass alone (ch_hamming_rank_scatter on prepared bases, limits of k = 1000).
2. Untouched paths against another build of the library (--parent-lib: the parent commit's, built from a checkout of it):
   hamming_topk k = 10 and evaluate() without radii, each library in a fresh process, the two alternating --procs times; every
   process reports its median round, and the medians over the processes must agree within +-3 % (the box-to-box spread README.md
   states) or the tool exits with status 1.  Beside each ratio stands the spread (largest / smallest process) of each library alone:
   the noise floor of that line.  One line is informational and does not decide the status: evaluate() at the small size is 0.35 ms of
   launches and host reads, and processes of ONE library differ by 13-26 % there, rounds of 0.8 s (2,000 calls) or not -- the figure
   belongs to the process, not to the library.  evaluate() is judged at 1M, where the scans dominate and the spread is 1-3 %."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--parent-lib", default="", help="libconcepthash_hip.so of the parent commit; without it part 2 is left out")
ap.add_argument("--lib", default="", help="(a leg of part 2) load this build of the library and print the untouched paths' times as JSON")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--procs", type=int, default=7)
ap.add_argument("--bound", type=float, default=0.03)
a = ap.parse_args()

SIZES = ((5794, 5994, 64), (16384, 1_000_000, 128))
NCLASS = 200
SMALL_CALLS = 400
INFORMATIONAL = ("evaluate 5794x5994x64",)     # see above: the spread inside one library is several times the bound


def clustered(torch, rows, nbit, centres, gen):
    labels = torch.randint(0, NCLASS, (rows,), device="cuda", generator=gen)
    return centres[labels] * 0.8 + 0.6 * torch.randn(rows, nbit, device="cuda", generator=gen), labels


def problem(torch, rt, Qn, G, nbit):
    gen = torch.Generator(device="cuda").manual_seed(1234 + nbit)
    centres = torch.sign(torch.randn(NCLASS, nbit, device="cuda", generator=gen))
    qc, ql = clustered(torch, Qn, nbit, centres, gen)
    gc, gl = clustered(torch, G, nbit, centres, gen)
    return rt.pack_sign(qc), rt.pack_sign(gc), ql, gl


def round_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def calls_for(Qn, G):
    """the small problem is a few launches long: SMALL_CALLS times the calls per round, so that a round is a fraction of a second and not a burst of host jitter"""
    return a.calls * (SMALL_CALLS if Qn * G < 1_000_000_000 else 1)


def interleaved(torch, variants, calls):
    """median round of every variant, the variants taking turns"""
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(a.rounds):
        for n, fn in variants.items():
            times[n].append(round_us(torch, fn, calls))
    return {n: statistics.median(v) for n, v in times.items()}


def leg():
    """one process of part 2: the untouched paths on the library at --lib"""
    import ctypes

    import torch                        # first: the library binds to the HIP runtime torch has loaded

    from concepthash_amd import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "ch_hamming_rank_scatter"):     # a build from before the entry existed
        del _lib.SIGNATURES["ch_hamming_rank_scatter"]
    from concepthash_amd import retrieval as rt
    out = {}
    for Qn, G, nbit in SIZES:
        q, g, ql, gl = problem(torch, rt, Qn, G, nbit)
        med = interleaved(torch, {"topk": lambda: rt.hamming_topk(q, g, 10), "evaluate": lambda: rt.evaluate(q, g, ql, gl)}, calls_for(Qn, G))
        out.update({f"{n} {Qn}x{G}x{nbit}": v for n, v in med.items()})
    print("LEG " + json.dumps(out))


def untouched_paths():
    libs = {"parent": os.path.abspath(a.parent_lib), "this": os.path.join(ROOT, "concepthash_amd", "libconcepthash_hip.so")}
    runs = {n: [] for n in libs}
    for _ in range(a.procs):
        for n, path in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", path, "--warmup", str(a.warmup), "--calls", str(a.calls),
                                "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=900)
            got = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
            if r.returncode != 0 or not got:
                raise SystemExit(f"leg '{n}' failed (status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[n].append(json.loads(got[0][4:]))
    lines = [f"untouched paths, this build against the parent commit's library: {a.procs} fresh processes per library, alternating; per process "
             f"the median of {a.rounds} rounds of {a.calls} calls ({SMALL_CALLS * a.calls} at the small size; us per call); bound +-{100 * a.bound:.0f} % on "
             f"the ratio of the medians over the processes (a line marked informational is not judged); spread = largest / smallest process of one library"]
    ok = True
    for key in runs["this"][0]:
        p, t = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        ratio = statistics.median(t) / statistics.median(p)
        good = abs(ratio - 1.0) <= a.bound
        judged = key not in INFORMATIONAL
        ok &= good or not judged
        lines.append(f"{key:34s} parent " + " ".join(f"{v:10.1f}" for v in p) + " | this " + " ".join(f"{v:10.1f}" for v in t) +
                     f" | this / parent {ratio:.4f} {('ok' if good else 'OUTSIDE THE BOUND') if judged else 'informational'}; spread parent {max(p) / min(p):.3f} this {max(t) / min(t):.3f}")
    return lines, ok


def new_paths():
    import torch
    from concepthash_amd import retrieval as rt
    lines = [f"{torch.cuda.get_device_name(0)}; clustered codes ({NCLASS} centres); median of {a.rounds} rounds of {a.calls} calls ({SMALL_CALLS * a.calls} at the small size) per variant, the "
             f"variants taking turns, after {a.warmup} warm-ups each; torch.cuda.Event around a round; us per call"]
    for Qn, G, nbit in SIZES:
        q, g, _, _ = problem(torch, rt, Qn, G, nbit)
        W = q.shape[1]
        seg = rt.map_seg_rows(Qn, G, W)
        _, base, counts = rt.bucket_counts(q, g, seg)
        within = counts.cumsum(1).double().mean(0)                      # mean rows within radius r
        radius = int((within - 300.0).abs().argmin())
        zq, zg = torch.zeros(Qn, dtype=torch.int32, device="cuda"), torch.zeros(G, dtype=torch.int32, device="cuda")
        k_s = min(1000, G)
        idx = torch.full((Qn * k_s,), -1, dtype=torch.int64, device="cuda")
        dist = torch.full((Qn * k_s,), -1, dtype=torch.int32, device="cuda")
        start = torch.arange(Qn, dtype=torch.int64, device="cuda") * k_s
        limit = torch.full((Qn,), k_s, dtype=torch.int64, device="cuda")
        med = interleaved(torch, {
            "hamming_topk k=10": lambda: rt.hamming_topk(q, g, 10),
            "hamming_topk k=128": lambda: rt.hamming_topk(q, g, 128),
            "hamming_ranked k=128": lambda: rt.hamming_ranked(q, g, 128),
            "hamming_ranked k=1000": lambda: rt.hamming_ranked(q, g, 1000),
            f"hamming_radius r={radius}": lambda: rt.hamming_radius(q, g, radius),
            "histogram pass": lambda: rt.hamming_hist(q, g, zq, zg, 0, seg),
            "scatter pass (limits 1000)": lambda: rt.rank_scatter(q, g, seg, base, start, limit, idx, dist, check=False)}, calls_for(Qn, G))
        lines.append(f"{Qn} x {G} x {nbit} bit, {-(-G // seg)} segments of {seg} rows; radius {radius} keeps {within[radius].item():.0f} rows per query on average "
                     f"(max {int(counts.cumsum(1)[:, radius].max())})")
        lines += [f"    {n:28s} {v:12.1f}" for n, v in med.items()]
        del base, idx, dist
    return lines


if a.lib:
    leg()
    sys.exit(0)
lines, ok = [], True
if a.parent_lib:                       # first: this process has not touched the GPU yet, each leg has it to itself
    lines, ok = untouched_paths()
    lines.append("")
lines = new_paths() + [""] + lines
text = "\n".join(lines).rstrip("\n") + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
sys.exit(0 if ok else 1)
