#!/usr/bin/env python3
"""The reduction (PCA / PCA-ITQ of the real-valued codes to a shorter code) on the GPU (profiles/search_pca_itq.txt, DESIGN.md section
2.0, "reduction"):
    python tools/pca_itq_report.py [--out FILE] [--sizes cub,1m] [--bits 32,16] [--blocks 4,1]
SYNTHETIC planted codes, the construction of tests/test_pca_gpu.py at scale: 4 blocks of 16 dimensions; per block 8 latent dimensions
of +-1 class centres plus N(0, sigma^2) beside 8 dimensions of N(0, 0.15^2), the block behind its own seeded orthogonal 16 x 16
matrix, plus 0.7.  The variance sits in directions no single bit owns, so dropping bits gives it up and a PCA finds it.  There is no
trained checkpoint offline: the retrieval numbers say how the fit behaves on this construction, not on a trained head.  Nothing here is
a pass mark.
Per size (CUB 5,794 x 5,994 x 64; 1,024 x 1M x 64; 200 classes), per number of blocks (4: one per concept; 1: one full PCA) and per
code length:
1. one `pca_moments` pass (sums and Gram of the shifted codes) and one `project_codes` over the database -- seconds, bytes per second
   (G n 4 / t: the pass over the real plane) and that rate against the 5.2 TB/s the adapter up-projection reaches at its traffic floor
   (0.65 of the 8 TB/s HBM peak); the Gram beside torch's fp32 `Y.T @ Y` on the same device (the full n x n
   product, whatever the blocks);
2. the whole fit (`fit_reduction`: two moment passes, eigh on the host in fp64, the projection, the rotation fit) beside the same fit
   in torch on the CPU (fp32 matmuls, the same eigh and SVDs; at most --cpu-iters updates of the rotation are run and scaled);
3. mAP@all of the Hamming ranking of the full / truncated (the first bits / blocks bits of every block) / PCA / PCA-ITQ codes, the
   plain codes shifted by the database mean.
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
PLANTED_BLOCKS, LATENT = 4, 8

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--sizes", default="cub,1m")
ap.add_argument("--bits", default="32,16")
ap.add_argument("--blocks", default="4,1")
ap.add_argument("--sigma", type=float, default=0.9)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--cpu-iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()

import torch  # noqa: E402

from concepthash_amd import retrieval as rt  # noqa: E402


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


def planted_codes(rows, n, nclass, seed, device):
    """-> (codes [rows, n] fp32, labels [rows] int64): the same centres and matrices for every seed, other rows"""
    s = n // PLANTED_BLOCKS
    fixed = torch.Generator().manual_seed(20240611)
    centres = [torch.where(torch.rand(nclass, LATENT, generator=fixed) < 0.5, -1.0, 1.0) for _ in range(PLANTED_BLOCKS)]
    Qs = [torch.linalg.qr(torch.randn(s, s, generator=fixed, dtype=torch.float64))[0].float() for _ in range(PLANTED_BLOCKS)]
    g = torch.Generator(device=device).manual_seed(seed)
    lab = torch.randint(0, nclass, (rows,), generator=g, device=device)
    cols = []
    for c, Q in zip(centres, Qs):
        z = torch.cat([c.to(device)[lab] + a.sigma * torch.randn(rows, LATENT, generator=g, device=device),
                       0.15 * torch.randn(rows, s - LATENT, generator=g, device=device)], dim=1)
        cols.append(z @ Q.to(device) + 0.7)
    return torch.cat(cols, dim=1).contiguous(), lab


def cpu_fit_seconds(x, bits, blocks, method, iters):
    """the same fit in torch on the CPU -> (seconds of the PCA part, seconds per update of the rotation)"""
    x = x.cpu()
    G, n = x.shape
    s, t = n // blocks, bits // blocks
    t0 = time.perf_counter()
    y = x - x.mean(0)
    yb = y.reshape(G, blocks, s).transpose(0, 1).contiguous()              # [blocks, G, s]
    C = (torch.bmm(yb.transpose(1, 2), yb).double() - yb.sum(1).double()[:, :, None] * yb.sum(1).double()[:, None, :] / G) / (G - 1)
    P, _ = rt.pca_components(C, t)
    v = torch.bmm(yb, P.float())
    t_pca = time.perf_counter() - t0
    if method != "pca-itq":
        return t_pca, 0.0
    R = torch.eye(t).repeat(blocks, 1, 1)
    t0 = time.perf_counter()
    for _ in range(iters):
        z = torch.bmm(v, R)
        B = torch.where(z > 0, 1.0, -1.0)
        U, _, Wh = torch.linalg.svd(torch.bmm(B.transpose(1, 2), v).double())
        R = (U @ Wh).transpose(1, 2).float()
    return t_pca, (time.perf_counter() - t0) / iters


lines = [f"{torch.cuda.get_device_name(0)}; timings: median of {a.rounds} rounds of {a.calls} calls after {a.warmup} warm-ups, torch.cuda.Event around a round",
         f"codes: SYNTHETIC -- {PLANTED_BLOCKS} blocks; per block {LATENT} latent dimensions of +-1 class centres plus N(0, {a.sigma}^2) beside the block's "
         "other dimensions of N(0, 0.15^2), behind a seeded orthogonal matrix, plus 0.7; the retrieval numbers describe this construction, not a trained head",
         f"rates: G n 4 bytes / seconds per pass, against {UP_PROJECTION_RATE / 1e12:.1f} TB/s (the adapter up-projection at its traffic floor, "
         "DESIGN.md section 3.8)"]
for name in a.sizes.split(","):
    Qn, G, n, C = SIZES[name]
    xq, ql = planted_codes(Qn, n, C, 1, "cuda")
    xg, gl = planted_codes(G, n, C, 2, "cuda")
    mean = xg.mean(0)
    xq, xg = (xq - mean).contiguous(), (xg - mean).contiguous()            # the plain codes: shifted by the database mean
    score = lambda q, g: rt.evaluate(rt.pack_sign(q.contiguous()), rt.pack_sign(g.contiguous()), ql, gl, R=-1, ks=(10,))["mAP"]
    lines.append("")
    lines.append(f"{name}: {Qn} x {G} x {n}, {C} classes")
    lines.append(f"  full {n} bits: mAP@all {score(xq, xg):.4f}")
    mu = (rt.pca_moments(xg, 1)[0] / G).float()
    t_mm = median_s(lambda: torch.matmul((xg - mu).T, xg - mu))
    t_mm_only = median_s(lambda: torch.matmul(xg.T, xg))
    lines.append(f"  torch fp32 (Y - mu).T @ (Y - mu) on the device: {t_mm * 1e6:.1f} us ({t_mm_only * 1e6:.1f} us for Y.T @ Y alone)")
    for blocks in [int(b) for b in a.blocks.split(",")]:
        s = n // blocks
        t_sum = median_s(lambda: rt._pca_moments(xg, n, s, None, 0, False))
        t_mom = median_s(lambda: rt.pca_moments(xg, blocks, mu))
        t_raw = median_s(lambda: rt._pca_moments(xg, n, s, mu, 0, True))
        rate = G * n * 4 / t_raw
        lines.append(f"  blocks = {blocks} (s = {s}):")
        lines.append(f"    sums alone {t_sum * 1e6:.1f} us; pca_moments {t_mom * 1e6:.1f} us with its finiteness check, {t_raw * 1e6:.1f} us without = "
                     f"{rate / 1e12:.3f} TB/s of codes = {rate / UP_PROJECTION_RATE:.3f} of the up-projection's rate; {t_raw / t_mm:.2f} x torch's matmul")
        for bits in [int(b) for b in a.bits.split(",")]:
            if bits % blocks or bits % PLANTED_BLOCKS:
                continue
            t = bits // blocks
            cols = (torch.arange(blocks)[:, None] * s + torch.arange(t)[None, :]).reshape(-1).cuda()
            out = {"truncated": score(xq[:, cols], xg[:, cols])}
            text = []
            for method in ("pca", "pca-itq"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fit = rt.fit_reduction(xg, bits, blocks, a.iters, method)
                torch.cuda.synchronize()
                t_fit = time.perf_counter() - t0
                Ac = rt.compact_projection(fit["A"], blocks)
                t_proj = median_s(lambda: rt._project_codes(xg, fit["mean"], Ac, n, s))
                prate = G * n * 4 / t_proj
                out[method] = score(rt.project_codes(xq, fit["mean"], fit["A"], blocks), rt.project_codes(xg, fit["mean"], fit["A"], blocks))
                t_pca, t_upd = cpu_fit_seconds(xg, bits, blocks, method, a.cpu_iters)
                updates = max(fit["iters_run"], 1) if method == "pca-itq" else 0
                text.append(f"      {method}: fit_reduction {t_fit:.3f} s ({fit['iters_run']} updates kept, explained {fit['explained_share']:.4f}, qerr "
                            f"{fit['qerr_pca']:.4f} -> {fit['qerr_after']:.4f}) | torch on the CPU: {t_pca:.3f} s PCA + {t_upd * 1e3:.1f} ms per update "
                            f"(measured over {a.cpu_iters}) = {t_pca + t_upd * a.iters:.2f} s for {a.iters} updates; project_codes {t_proj * 1e6:.1f} us = "
                            f"{prate / 1e12:.3f} TB/s of codes = {prate / UP_PROJECTION_RATE:.3f} of the up-projection's rate")
            lines.append(f"    {bits} bits (t = {t}): mAP@all truncated {out['truncated']:.4f}  PCA {out['pca']:.4f}  PCA-ITQ {out['pca-itq']:.4f}  "
                         f"(PCA-ITQ - truncated {out['pca-itq'] - out['truncated']:+.4f})")
            lines.extend(text)
    del xq, xg
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
