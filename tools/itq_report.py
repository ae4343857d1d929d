#!/usr/bin/env python3
"""The learned rotation (iterative quantisation) on the GPU (profiles/search_itq.txt, DESIGN.md section 2.0, "learned rotation"):
    python tools/itq_report.py [--out FILE] [--sizes cub,1m] [--blocks 4,1]
Clustered SYNTHETIC codes (`concepthash_amd.synthetic.synthetic_real_codes`: class centres +-1 plus N(0, 0.78^2), both sides) behind a
PLANTED rotation: every quarter of the code (16 dimensions at 64) is rotated by its own seeded orthogonal matrix, so sign() of the codes as
they stand loses what a block-diagonal rotation can give back.  There is no trained checkpoint offline: the retrieval numbers say how
the fit behaves on this construction, not on a trained head.
Per size (CUB 5,794 x 5,994 x 64; 1,024 x 1M x 64; 200 classes) and per number of blocks (4: one per concept; 1: one full rotation):
1. one `itq_step` over the database -- seconds per step, its bytes per second (G n 4 / t: the pass over the real plane) and that rate
   against the 5.2 TB/s the adapter up-projection reaches at its traffic floor (0.65 of the 8 TB/s HBM peak) --
   and one `rotate_codes` over it;
2. the whole fit (`fit_rotation`, 50 updates at most: the passes on the GPU, the SVDs of the blocks on the host in fp64) beside the
   same fit in torch on the CPU (fp32 matmuls, the same SVDs; at most --cpu-iters updates of it are run and the time per update is scaled);
3. the quantisation error of the database and mAP@all, P@10, R@10 of the Hamming ranking before and after (queries rotated as well).
Timings: median of --rounds rounds of --calls calls after --warmup warm-ups, torch.cuda.Event around a round."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"cub": (5794, 5994, 64, 200), "1m": (1024, 1_000_000, 64, 200)}
UP_PROJECTION_RATE = 0.65 * 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--sizes", default="cub,1m")
ap.add_argument("--blocks", default="4,1")
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--cpu-iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()

import torch  # noqa: E402

from concepthash_amd import retrieval as rt  # noqa: E402
from concepthash_amd.synthetic import synthetic_real_codes  # noqa: E402

KS = (1, 5, 10)
PLANTED_BLOCKS = 4


def median_s(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3 / a.calls)
    return statistics.median(times)


def planted(n, device):
    """block-diagonal, PLANTED_BLOCKS seeded orthogonal blocks"""
    g = torch.Generator().manual_seed(20240607)
    s = n // PLANTED_BLOCKS
    return torch.block_diag(*[torch.linalg.qr(torch.randn(s, s, generator=g, dtype=torch.float64))[0] for _ in range(PLANTED_BLOCKS)]).float().to(device)


def cpu_fit_seconds_per_update(x, blocks, iters):
    """the same loop in torch on the CPU: rotate, sign, B^T V per block (fp32), SVD (fp64), R = W U^T"""
    x = x.cpu()
    G, n = x.shape
    s = n // blocks
    xb = x.reshape(G, blocks, s).transpose(0, 1).contiguous()             # [blocks, G, s]
    R = torch.eye(s).repeat(blocks, 1, 1)
    t0 = time.perf_counter()
    for _ in range(iters):
        z = torch.bmm(xb, R)
        B = torch.where(z > 0, 1.0, -1.0)
        U, _, Wh = torch.linalg.svd(torch.bmm(B.transpose(1, 2), xb).double())
        R = (U @ Wh).transpose(1, 2).float()
    return (time.perf_counter() - t0) / iters


def row(name, r, qerr):
    return f"    {name:10s} qerr {qerr:.4f}  mAP@all {r['mAP']:.4f}  P@10 {r['precisions'][2]:.4f}  R@10 {r['recalls'][2]:.4f}"


lines = [f"{torch.cuda.get_device_name(0)}; timings: median of {a.rounds} rounds of {a.calls} calls after {a.warmup} warm-ups, torch.cuda.Event around a round",
         f"codes: SYNTHETIC -- class centres +-1 plus N(0, 0.78^2) (concepthash_amd.synthetic.synthetic_real_codes), each of {PLANTED_BLOCKS} blocks behind its "
         "own seeded orthogonal matrix; the retrieval numbers describe this construction, not a trained head",
         f"step rate: G n 4 bytes / seconds per step, against {UP_PROJECTION_RATE / 1e12:.1f} TB/s (the adapter up-projection at its traffic floor, "
         "DESIGN.md section 3.8)"]
for name in a.sizes.split(","):
    Qn, G, n, C = SIZES[name]
    P = planted(n, "cuda")
    xq, ql = synthetic_real_codes(Qn, n, seed=1, nclass=C, device="cuda")
    xg, gl = synthetic_real_codes(G, n, seed=2, nclass=C, device="cuda")
    clean = rt.evaluate(rt.pack_sign(xq), rt.pack_sign(xg), ql, gl, R=-1, ks=KS)
    xq, xg = (xq @ P).contiguous(), (xg @ P).contiguous()
    lines.append("")
    lines.append(f"{name}: {Qn} x {G} x {n}, {C} classes")
    lines.append(row("unrotated", clean, rt.itq_step(xg @ P.T, torch.eye(n, device="cuda"), 1)[2]) + "   (the codes in front of the planted rotation)")
    for blocks in [int(b) for b in a.blocks.split(",")]:
        s = n // blocks
        R0 = torch.eye(s, device="cuda").repeat(blocks, 1)
        t_step = median_s(lambda: rt.itq_step(xg, R0, blocks))
        t_rot = median_s(lambda: rt.rotate_codes(xg, R0, blocks))
        rate = G * n * 4 / t_step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = rt.fit_rotation(xg, blocks, a.iters)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        passes = len(fit["l1"])
        t_cpu = cpu_fit_seconds_per_update(xg, blocks, a.cpu_iters)
        before = rt.evaluate(rt.pack_sign(xq), rt.pack_sign(xg), ql, gl, R=-1, ks=KS)
        after = rt.evaluate(rt.pack_sign(rt.rotate_codes(xq, fit["R"], blocks)), rt.pack_sign(rt.rotate_codes(xg, fit["R"], blocks)), ql, gl, R=-1, ks=KS)
        lines.append(f"  blocks = {blocks} (s = {s}):")
        lines.append(f"    itq_step {t_step * 1e6:.1f} us per step = {rate / 1e12:.3f} TB/s of codes = {rate / UP_PROJECTION_RATE:.3f} of the up-projection's rate; "
                     f"rotate_codes {t_rot * 1e6:.1f} us")
        lines.append(f"    fit_rotation: {passes} passes, best after {fit['iters_run']} updates, {t_fit:.3f} s in all ({t_fit / passes * 1e3:.2f} ms per pass with its "
                     f"host SVD) | torch on the CPU: {t_cpu * 1e3:.1f} ms per update (measured over {a.cpu_iters}), {t_cpu * passes:.2f} s for as many")
        lines.append(row("before", before, fit["qerr_before"]))
        lines.append(row("after", after, fit["qerr_after"]) + f"   mAP {after['mAP'] - before['mAP']:+.4f}")
    del xq, xg
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
