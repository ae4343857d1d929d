#!/usr/bin/env python3
"""Weighted (asymmetric) against plain Hamming top-k (profiles/search_weighted_topk.txt):
    python tools/weighted_topk_bench.py [--out FILE] [--asm FILE.s]
1. Registers: VGPRs and scratch bytes of every unfiltered topk_weighted_partial_kernel<W, KREG, P, TopkNoFilter> instance, from the code-object metadata
   (`amdhsa.kernels`) of csrc/hamming_topk.hip compiled to assembly for gfx950 -- compiled here, or read from --asm.
2. Timing: hamming_topk, hamming_topk_weighted with 4-bit and with 8-bit weights, k = 10, at 5,794 x 5,994 x 64 bit and
   16,384 x 1M x 128 bit; one process, the three variants taking turns over --rounds rounds of --calls calls each (torch.cuda.Event
   around a round's calls, warm-ups excluded); the median round in microseconds per call and the ratios to the unweighted scan.
3. Ties: the share of queries whose 10th hit has the distance of the 11th (a top-11 call), for uniform codes and for clustered
   ones (200 class centres, codes = centre * 0.8 + N(0, 0.6)), under the Hamming ranking and under both weighted ones."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--asm", default="", help="assembly of csrc/hamming_topk.hip (hipcc --cuda-device-only -S); default: compile it")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-timing", action="store_true", help="the register table only (needs no GPU)")
a = ap.parse_args()


def register_table(asm_path):
    from concepthash_amd import build
    if not asm_path:
        tmp = tempfile.mkdtemp()
        asm_path = os.path.join(tmp, "hamming_topk.s")
        subprocess.run([build._hipcc()] + build.FLAGS + ["-I", build.CSRC, "--cuda-device-only", "-S", "-o", asm_path,
                        os.path.join(build.CSRC, "hamming_topk.hip")], check=True, capture_output=True)
    text = open(asm_path).read()
    meta = text[text.index("amdhsa.kernels:"):]
    rows = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        field = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", blk).group(1))
        m = re.search(r"topk_weighted_partial_kernelILi(\d+)ELi(\d+)ELi(\d+)ENS_12TopkNoFilterEE", blk)   # the unfiltered instances
        if m:
            W, kreg, P = (int(v) for v in m.groups())
            rows[(P, W, kreg)] = (field("vgpr_count"), int(re.match(r"\s*(\d+)", blk).group(1)), field("sgpr_count"),
                                  field("private_segment_fixed_size"), field("vgpr_spill_count"))
    lines = ["topk_weighted_partial_kernel<W, KREG, P, TopkNoFilter>: registers from the code-object metadata (vgpr_count includes the AGPRs)",
             "  P  W  KREG  VGPRs  of which AGPRs  SGPRs  scratch bytes  spilled VGPRs"]
    for (P, W, kreg), (v, ag, s, scratch, spill) in sorted(rows.items()):
        lines.append(f"  {P}  {W}  {kreg:4d}  {v:5d}  {ag:14d}  {s:5d}  {scratch:13d}  {spill:13d}")
    lines.append(f"{len(rows)} instances, {sum(1 for r in rows.values() if r[3] or r[4])} with scratch or spills")
    return lines


lines = register_table(a.asm)
if not a.no_timing:
    import torch

    from concepthash_amd import retrieval as rt
    gen = torch.Generator(device="cuda").manual_seed(1234)

    def randn(rows, nbit):
        return torch.randn(rows, nbit, device="cuda", generator=gen)

    def round_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    lines.append("")
    lines.append(f"{torch.cuda.get_device_name(0)}; k = 10; median of {a.rounds} rounds of {a.calls} calls per variant, the variants taking turns, "
                 f"after {a.warmup} warm-ups each; torch.cuda.Event around a round")
    for Qn, G, nbit in ((5794, 5994, 64), (16384, 1_000_000, 128)):
        codes = randn(Qn, nbit)
        q, g = rt.pack_sign(codes), rt.pack_sign(randn(G, nbit))
        p4, p8 = rt.weight_planes(codes, 4)[0], rt.weight_planes(codes, 8)[0]
        variants = {"hamming_topk": lambda: rt.hamming_topk(q, g, 10), "weighted, 4-bit": lambda: rt.hamming_topk_weighted(q, p4, g, 10),
                    "weighted, 8-bit": lambda: rt.hamming_topk_weighted(q, p8, g, 10)}
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n in variants}
        for _ in range(a.rounds):
            for n, fn in variants.items():
                times[n].append(round_us(fn))
        med = {n: statistics.median(v) for n, v in times.items()}
        planes_us = round_us(lambda: rt.weight_planes(codes, 8))
        lines.append(f"{Qn} x {G} x {nbit} bit: " + " | ".join(f"{n} {med[n]:10.1f} us ({med[n] / med['hamming_topk']:.2f}x)" for n in variants) +
                     f" | weight_planes (8-bit) {planes_us:.1f} us")

    lines.append("")
    lines.append("share of queries whose 10th hit ties with the 11th (top-11 call), 1,024 queries x 5,994 rows")
    for nbit in (64, 128):
        for kind in ("uniform", "clustered"):
            if kind == "uniform":
                qc, gc = randn(1024, nbit), randn(5994, nbit)
            else:
                centres = torch.sign(randn(200, nbit))
                qc = centres[torch.randint(0, 200, (1024,), device="cuda", generator=gen)] * 0.8 + 0.6 * randn(1024, nbit)
                gc = centres[torch.randint(0, 200, (5994,), device="cuda", generator=gen)] * 0.8 + 0.6 * randn(5994, nbit)
            q, g = rt.pack_sign(qc), rt.pack_sign(gc)
            share = {}
            _, d = rt.hamming_topk(q, g, 11)
            share["hamming"] = (d[:, 9] == d[:, 10]).float().mean().item()
            for bits in (4, 8):
                _, d = rt.hamming_topk_weighted(q, rt.weight_planes(qc, bits)[0], g, 11)
                share[f"weighted, {bits}-bit"] = (d[:, 9] == d[:, 10]).float().mean().item()
            lines.append(f"{nbit} bit, {kind:9s}: " + " | ".join(f"{n} {100 * v:5.1f} %" for n, v in share.items()))
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
