#!/usr/bin/env python3
"""Two-stage search -- a Hamming shortlist ordered by a dense distance -- beside its two ends (profiles/search_rerank.txt, DESIGN.md
section 2.0, "two-stage"):
    python tools/rerank_report.py [--out FILE] [--sizes cub,1m] [--metric cosine] [--parent-lib PATH/libconcepthash_hip.so]
Clustered SYNTHETIC codes, those of tools/dense_report.py (`concepthash_amd.synthetic.synthetic_real_codes`: class centres +-1 plus
N(0, 0.78^2), both sides) -- there is no trained checkpoint offline, so agreement and mAP say how the lists behave on this noise model,
not on a trained head.  Per size (CUB 5,794 x 5,994 x 64; 1,024 x 1M x 64; 200 classes) and shortlist m in 100, 1000, 4096:
1. time of the two stages apart -- `hamming_ranked` at depth m, and ch_dense_rerank on that shortlist at k = 10 (the entry alone, on
   checked codes and preallocated outputs; `dense_rerank`, the wrapper, beside it: it also checks that the codes are finite, one pass
   over the gallery) -- beside `hamming_topk` and `dense_topk` at k = 10;
2. the rerank stage's bytes per second against the HBM rate: the shortlisted rows (n x 4 bytes each), the candidate ids and the output
   lists over the entry's time; 8.0 TB/s is the part's peak, 6.3 TB/s what a float4 copy reaches;
3. agreement@10 (the mean share of the exhaustive dense top-10 found in the two-stage top-10) and mAP@m, P@10 under the Hamming
   ranking, the two-stage list and the exhaustive dense ranking.
No threshold is set on any of these figures.
4. With --parent-lib: `dense_topk` (k = 10) and `ch_dense_prepare` of the gallery, whose kernel this change touched, against the parent
   commit's library by the procedure of tools/ranked_list_bench.py: each library in a fresh process, the two alternating --procs times,
   +-3 % on the ratio of the medians over the processes, or the tool exits with status 1.
One process per part, the variants taking turns over --rounds rounds of --calls calls each after --warmup warm-ups, HIP events
(torch.cuda.Event) around a round; the median round in microseconds per call."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"cub": (5794, 5994, 64, 200), "1m": (1024, 1_000_000, 64, 200)}
SHORTLISTS = (100, 1000, 4096)
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--sizes", default="cub,1m")
ap.add_argument("--metric", default="cosine")
ap.add_argument("--parent-lib", default="", help="libconcepthash_hip.so of the parent commit; without it part 4 is left out")
ap.add_argument("--lib", default="", help="(a leg of part 4) load this build of the library and print the touched paths' times as JSON")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--procs", type=int, default=3)
ap.add_argument("--bound", type=float, default=0.03)
a = ap.parse_args()


def medians(torch, variants):
    """the variants taking turns -> {name: median round, us per call}"""
    def round_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(a.rounds):
        for n, fn in variants.items():
            times[n].append(round_us(fn))
    return {n: statistics.median(v) for n, v in times.items()}


def leg():
    """one process of part 4: the touched paths on the library at --lib"""
    import ctypes

    import torch                        # first: the library binds to the HIP runtime torch has loaded

    from concepthash_amd import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "ch_dense_rerank"):       # a build from before the entry existed
        del _lib.SIGNATURES["ch_dense_rerank"]
    from concepthash_amd import retrieval as rt
    from concepthash_amd.synthetic import synthetic_real_codes
    out = {}
    for name in a.sizes.split(","):
        Qn, G, n, C = SIZES[name]
        xq, _ = synthetic_real_codes(Qn, n, seed=1, nclass=C, device="cuda")
        xg, _ = synthetic_real_codes(G, n, seed=2, nclass=C, device="cuda")
        pq, pg = rt.prepare_dense(xq, a.metric), rt.prepare_dense(xg, a.metric)
        lib = _lib.load()
        prepared = torch.empty_like(pg.data)
        med = medians(torch, {"dense_topk k=10": lambda: rt.dense_topk(pq, pg, a.metric, 10),
                              "ch_dense_prepare (gallery)": lambda: lib.ch_dense_prepare(_lib.ptr(xg), G, n, rt.dense_metric_id(a.metric), _lib.ptr(prepared),
                                                                                         _lib.stream_ptr())})
        out.update({f"{k} {a.metric} {Qn}x{G}x{n}": v for k, v in med.items()})
    print("LEG " + json.dumps(out))


def touched_paths():
    libs = {"parent": os.path.abspath(a.parent_lib), "this": os.path.join(ROOT, "concepthash_amd", "libconcepthash_hip.so")}
    runs = {n: [] for n in libs}
    for _ in range(a.procs):
        for n, path in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", path, "--warmup", str(a.warmup), "--calls", str(a.calls),
                                "--rounds", str(a.rounds), "--sizes", a.sizes, "--metric", a.metric], capture_output=True, text=True, timeout=900)
            got = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
            if r.returncode != 0 or not got:
                raise SystemExit(f"leg '{n}' failed (status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[n].append(json.loads(got[0][4:]))
    lines = [f"paths whose file this change touched (dense_prepare_kernel now normalises through dense_row_scale), this build against the parent "
             f"commit's library: {a.procs} fresh processes per library, alternating; per process the median of {a.rounds} rounds of {a.calls} calls "
             f"(us per call); bound +-{100 * a.bound:.0f} % on the ratio of the medians over the processes; spread = largest / smallest process of "
             f"one library"]
    ok = True
    for key in runs["this"][0]:
        p, t = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        ratio = statistics.median(t) / statistics.median(p)
        good = abs(ratio - 1.0) <= a.bound
        ok &= good
        lines.append(f"{key:48s} parent " + " ".join(f"{v:9.1f}" for v in p) + " | this " + " ".join(f"{v:9.1f}" for v in t) +
                     f" | this / parent {ratio:.4f} {'ok' if good else 'OUTSIDE THE BOUND'}; spread parent {max(p) / min(p):.3f} this {max(t) / min(t):.3f}")
    return lines, ok


def two_stage():
    import torch

    from concepthash_amd import _lib
    from concepthash_amd import retrieval as rt
    from concepthash_amd.synthetic import synthetic_real_codes
    metric, mid = a.metric, rt.dense_metric_id(a.metric)
    lib = _lib.load()
    lines = [f"{torch.cuda.get_device_name(0)}; metric {metric}; timings: median of {a.rounds} rounds of {a.calls} calls per variant, the variants "
             f"taking turns, after {a.warmup} warm-ups each; torch.cuda.Event around a round; microseconds per call",
             "codes: SYNTHETIC -- class centres +-1 plus N(0, 0.78^2) on both sides (concepthash_amd.synthetic.synthetic_real_codes); no trained "
             "checkpoint exists here, so agreement and mAP describe this noise model, not a trained head",
             f"bytes of the rerank stage: shortlisted rows x n x 4 + ids x 8 + outputs x 12; HBM {HBM_PEAK / 1e12:.1f} TB/s peak, "
             f"{HBM_COPY / 1e12:.1f} TB/s reached by a float4 copy"]
    for name in a.sizes.split(","):
        Qn, G, n, C = SIZES[name]
        xq, ql = synthetic_real_codes(Qn, n, seed=1, nclass=C, device="cuda")
        xg, gl = synthetic_real_codes(G, n, seed=2, nclass=C, device="cuda")
        q, g = rt.pack_sign(xq), rt.pack_sign(xg)
        pq, pg = rt.prepare_dense(xq, metric), rt.prepare_dense(xg, metric)
        lines += ["", f"{name}: {Qn} x {G} x {n}, {C} classes"]
        ends = medians(torch, {"hamming_topk k=10": lambda: rt.hamming_topk(q, g, 10), "dense_topk k=10": lambda: rt.dense_topk(pq, pg, metric, 10)})
        lines.append("  the two ends: " + " | ".join(f"{k} {v:.1f} us" for k, v in ends.items()))
        for m in SHORTLISTS:
            cand, _ = rt.hamming_ranked(q, g, m)
            k = 10
            idx = torch.empty(Qn, k, dtype=torch.int64, device="cuda")
            dist = torch.empty(Qn, k, dtype=torch.float32, device="cuda")

            def entry():
                _lib.check(lib.ch_dense_rerank(_lib.ptr(xq), Qn, _lib.ptr(xg), G, n, mid, _lib.ptr(cand), m, k, 0, _lib.ptr(idx), _lib.ptr(dist),
                                               _lib.stream_ptr()), "ch_dense_rerank")
            t = medians(torch, {"shortlist": lambda: rt.hamming_ranked(q, g, m), "rerank entry": entry,
                                "rerank wrapper": lambda: rt.dense_rerank(xq, xg, cand, metric, k, validate=False)})
            filled = int((cand >= 0).sum())
            moved = filled * n * 4 + cand.numel() * 8 + Qn * k * 12 + Qn * n * 4
            rate = moved / (t["rerank entry"] * 1e-6)
            both = t["shortlist"] + t["rerank entry"]
            lines.append(f"  m = {m}: shortlist (hamming_ranked) {t['shortlist']:.1f} us | rerank (ch_dense_rerank, k = 10) {t['rerank entry']:.1f} us | "
                         f"dense_rerank wrapper {t['rerank wrapper']:.1f} us | both stages {both:.1f} us = {both / ends['hamming_topk k=10']:.2f}x "
                         f"hamming_topk, {both / ends['dense_topk k=10']:.2f}x dense_topk")
            lines.append(f"      rerank: {moved / 1e6:.1f} MB in {t['rerank entry']:.1f} us = {rate / 1e12:.3f} TB/s, {100 * rate / HBM_PEAK:.1f} % of the peak, "
                         f"{100 * rate / HBM_COPY:.1f} % of a copy")
            meff = min(m, G)
            ks = (1, 5, 10)
            two = rt.evaluate_reranked(xq, xg, ql, gl, metric, m, R=meff, ks=ks, q_packed=q, g_packed=g)
            ham = rt.evaluate(q, g, ql, gl, R=meff, ks=ks)
            full = rt.evaluate_dense(xq, xg, ql, gl, metric, R=meff, ks=ks)
            lines.append(f"      agreement@10 {two['agreement'][10]:.4f} | mAP@{meff}: hamming {ham['mAP']:.4f}, two-stage {two['mAP']:.4f}, exhaustive "
                         f"{metric} {full['mAP']:.4f} | P@10: {ham['precisions'][2]:.4f}, {two['precisions'][2]:.4f}, {full['precisions'][2]:.4f}")
            del cand, idx, dist
        del xq, xg, q, g, pq, pg
    return lines


if a.lib:
    leg()
    sys.exit(0)
lines, ok = [], True
if a.parent_lib:                       # first: this process has not touched the GPU yet, each leg has it to itself
    lines, ok = touched_paths()
lines = two_stage() + ([""] + lines if lines else [])
text = "\n".join(lines).rstrip("\n") + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
sys.exit(0 if ok else 1)
