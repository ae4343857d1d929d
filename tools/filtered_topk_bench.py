#!/usr/bin/env python3
"""Filtered against unfiltered top-k (profiles/search_filtered_topk.txt, DESIGN.md section 2.0, "filtered search"):
    python tools/filtered_topk_bench.py [--out FILE] [--asm-dir DIR] [--parent-src DIR | --parent-asm-dir DIR] [--parent-lib LIB]
1. Registers (no GPU): VGPRs, SGPRs, scratch bytes and code bytes of every filtered scan instance beside its unfiltered sibling, from
   what the compiler reports for csrc/hamming_topk.hip and csrc/hamming_ternary.hip compiled to gfx950 assembly -- compiled here, or
   read from --asm-dir (hamming_topk.s, hamming_ternary.s) -- and the workgroups per CU that the segment rules derive from them.
   A scan instance is known by its mangled name: the kernel template, its integer arguments and the filter, a template argument of
   type TopkFilter or TopkNoFilter (in sources from before that: a _filtered_kernel of its own).
2. The kernels of the parent (no GPU): with --parent-src (the csrc directory of the parent commit, compiled here) or --parent-asm-dir,
   the register counts and code sizes of every kernel the parent has, parent against this build, a scan instance matched to its
   successor by (family, template arguments, filtered or not) and not by name.  The scans are meant to be equal.
3. Timing (--no-timing leaves it out): at 5,794 x 5,994 x 64 bit and 1,024 x 1M x 64 bit, k = 10 and k = 128, one process, the variants
   taking turns over --rounds rounds of --calls calls each (torch.cuda.Event around a round's calls, warm-ups excluded), the median
   round in microseconds per call: unfiltered, filtered with every row admitted, allow-lists of density 0.5 / 0.1 / 0.01 with random
   rows and with runs of 64 rows, a group filter alone (exclude by row; only, over 200 groups), and the post-filter a user has today
   (unfiltered k = 128, filtered on the host) with the share of the requested k it still delivers.
4. With --parent-lib (the parent commit's libconcepthash_hip.so): every top-k entry, unfiltered and filtered, topk_merge and the dense
   top-k of this build against the parent's, the two libraries taking turns in this process behind the same Python; beside each
   median the parent's own spread over its rounds (max - min), the margin a difference has to exceed to mean anything."""
import argparse
import ctypes
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
ap.add_argument("--asm-dir", default="", help="hamming_topk.s and hamming_ternary.s of this build (hipcc --cuda-device-only -S); default: compile")
ap.add_argument("--parent-src", default="", help="the parent commit's concepthash_amd/csrc: its two scan sources are compiled for the comparison")
ap.add_argument("--parent-asm-dir", default="", help="... or their assembly")
ap.add_argument("--parent-lib", default="", help="the parent commit's library: the untouched entries are timed against it")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-timing", action="store_true", help="the register tables only (needs no GPU)")
a = ap.parse_args()

SOURCES = ("hamming_topk", "hamming_ternary")
KERNEL_INFO = re.compile(r"\.set (\S+)\.has_indirect_call, \d+\n\s*\.section\s+\.AMDGPU\.csdata[^\n]*\n; Kernel info:\n; codeLenInByte = (\d+)\n"
                         r"; TotalNumSgprs: (\d+)\n; NumVgprs: (\d+)\n; NumAgprs: (\d+)\n; TotalNumVgprs: (\d+)\n; ScratchSize: (\d+)\n")


def assembly(csrc, asm_dir):
    """{source: assembly text} of SOURCES under `csrc`, compiled unless asm_dir holds them"""
    from concepthash_amd import build
    out = {}
    for src in SOURCES:
        if asm_dir:
            path = os.path.join(asm_dir, src + ".s")
        else:
            path = os.path.join(tempfile.mkdtemp(), src + ".s")
            subprocess.run([build._hipcc()] + build.FLAGS + ["-I", csrc, "--cuda-device-only", "-S", "-o", path, os.path.join(csrc, src + ".hip")],
                           check=True, capture_output=True)
        out[src] = open(path).read()
    return out


def kernels(asm):
    """{mangled name: dict(code, sgprs, vgprs, agprs, total_vgprs, scratch)} of every kernel of the two sources"""
    rows = {}
    for text in asm.values():
        for m in KERNEL_INFO.finditer(text):
            code, sg, vg, ag, tv, scr = (int(v) for v in m.groups()[1:])
            rows[m.group(1)] = dict(code=code, sgprs=sg, vgprs=vg, agprs=ag, total_vgprs=tv, scratch=scr)
    return rows


def per_cu(vgprs):
    """workgroups of four waves per CU: topk_per_cu of csrc/hamming_shared.h, the one statement of the rule"""
    return max(1, min(8, 512 // max(8, (vgprs + 7) // 8 * 8)))


FAMILIES = (   # (what, the kernel template, the meaning of its template arguments in front of the filter)
    ("plain / masked", "topk_partial", "W, KREG, MASKED"),
    ("weighted", "topk_weighted_partial", "W, KREG, P"),
    ("ternary", "topk_ternary_partial", "W, KREG"),
)
SCAN = re.compile(r"\d+(topk_(?:weighted_|ternary_)?partial)(_filtered)?_kernelI((?:L[ib]\d+E)+)(?:NS_\d+(Topk(?:No)?Filter)E)?E")


def scan_instance(name):
    """(family, template arguments, filtered) of a scan kernel's mangled name -- the filter a template argument of type TopkFilter or
    TopkNoFilter or, in sources from before that, a _filtered_kernel of its own -- or None for any other kernel"""
    m = SCAN.search(name)
    if m is None:
        return None
    return m.group(1), tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(3))), bool(m.group(2)) or m.group(4) == "TopkFilter"


def register_tables(mine):
    lines = ["Registers of the filtered scan instances beside their unfiltered siblings, as the compiler reports them for gfx950",
             "(TotalNumVgprs includes the AGPRs; wg/CU = workgroups of four waves per CU, min(8, 512 / VGPRs rounded up to 8))"]
    scratch = steps = count = 0
    for what, family, args in FAMILIES:
        lines.append(f"{what}: <{args}>   VGPRs plain -> filtered   SGPRs plain -> filtered   scratch   code bytes plain -> filtered   wg/CU")
        table = {}
        for name, r in mine.items():
            inst = scan_instance(name)
            if inst is not None and inst[0] == family:
                table.setdefault(inst[1], [None, None])[inst[2]] = r
        for t, (p, f) in sorted(table.items()):
            if p is None or f is None:
                raise SystemExit(f"{what} {t}: an instance without its sibling")
            count += 1
            scratch += f["scratch"] != 0 or p["scratch"] != 0
            a_, b_ = per_cu(p["total_vgprs"]), per_cu(f["total_vgprs"])
            steps += a_ != b_
            lines.append(f"  {str(t):14s} {p['total_vgprs']:4d} -> {f['total_vgprs']:4d}   {p['sgprs']:4d} -> {f['sgprs']:4d}   {f['scratch']:4d}   "
                         f"{p['code']:6d} -> {f['code']:6d}   {a_} -> {b_}" + ("   <- another step" if a_ != b_ else ""))
    lines.append(f"{count} filtered instances, {scratch} with scratch, {steps} on another residency step than their sibling")
    return lines


def parent_comparison(mine, theirs):
    """every kernel of the parent against its successor: a scan instance is matched by (family, template arguments, filtered or not)
    -- its name may have changed --, any other kernel by its mangled name"""
    def key(name):
        return scan_instance(name) or name

    def show(k):
        return k if isinstance(k, str) else f"{k[0]}_kernel<{', '.join(str(v) for v in k[1])}>" + (" filtered" if k[2] else "")

    lines = ["", "The kernels the parent commit has, parent -> this build (code bytes, SGPRs, VGPRs, scratch)"]
    successors = {key(name): r for name, r in mine.items()}
    differ = scans = 0
    for k, p in sorted(((key(name), r) for name, r in theirs.items()), key=lambda kv: (isinstance(kv[0], str), kv[0])):
        scans += not isinstance(k, str)
        m = successors.get(k)
        if m is None:
            lines.append(f"  {show(k)}: not in this build")
        else:
            lines.append(f"  {show(k)}: {p['code']} -> {m['code']} B, {p['sgprs']} -> {m['sgprs']} SGPRs, {p['total_vgprs']} -> {m['total_vgprs']} VGPRs, "
                         f"scratch {p['scratch']} -> {m['scratch']}" + ("" if m == p else "   <- differs"))
        differ += m != p
    lines.append(f"{len(theirs)} kernels of the parent ({scans} scan instances), {differ} differ in this build "
                 f"({len(set(successors) - set(key(n) for n in theirs))} kernels are new)")
    return lines


from concepthash_amd import build as _build

mine = kernels(assembly(_build.CSRC, a.asm_dir))
lines = register_tables(mine)
if a.parent_src or a.parent_asm_dir:
    lines += parent_comparison(mine, kernels(assembly(a.parent_src, a.parent_asm_dir)))

if not a.no_timing:
    import torch

    from concepthash_amd import _lib, retrieval as rt
    gen = torch.Generator(device="cuda").manual_seed(1234)

    def rand(rows, W):
        return torch.randint(-2 ** 63, 2 ** 63 - 1, (rows, W), dtype=torch.int64, device="cuda", generator=gen)

    def round_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    def interleaved(variants, rounds=False):
        """{variant: its median round}, or with rounds=True {variant: every round}"""
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n in variants}
        for r in range(a.rounds):   # every other round backwards: no variant always runs behind the same neighbour's cache state
            for n, fn in list(variants.items())[::-1 if r % 2 else 1]:
                times[n].append(round_us(fn))
        return times if rounds else {n: statistics.median(v) for n, v in times.items()}

    lines += ["", f"{torch.cuda.get_device_name(0)}; median of {a.rounds} rounds of {a.calls} calls per variant, the variants taking turns, after "
                  f"{a.warmup} warm-ups each; torch.cuda.Event around a round; microseconds per call (ratio to the unfiltered scan)"]
    for Qn, G in ((5794, 5994), (1024, 1_000_000)):
        q, g = rand(Qn, 1), rand(G, 1)
        rows = torch.arange(G, device="cuda")
        allows = {"every row": torch.ones(G, dtype=torch.bool, device="cuda")}
        for dens in (0.5, 0.1, 0.01):
            allows[f"random {dens}"] = torch.rand(G, device="cuda", generator=gen) < dens
            allows[f"runs of 64 {dens}"] = (torch.rand((G + 63) // 64, device="cuda", generator=gen) < dens)[rows >> 6]
        bitmaps = {n: rt.row_bitmap(v) for n, v in allows.items()}
        group200 = torch.randint(0, 200, (G,), dtype=torch.int32, device="cuda", generator=gen)
        want_row = torch.randint(0, G, (Qn,), dtype=torch.int64, device="cuda", generator=gen)
        want_grp = torch.randint(0, 200, (Qn,), dtype=torch.int64, device="cuda", generator=gen)
        for k in (10, 128):
            variants = {"unfiltered": lambda: rt.hamming_topk(q, g, k)}
            for n, bm in bitmaps.items():
                variants[f"allow, {n}"] = (lambda bm: lambda: rt.hamming_topk_filtered(q, g, k, allow=bm))(bm)
            variants["group: exclude by row"] = lambda: rt.hamming_topk_filtered(q, g, k, want=want_row, exclude=True)
            variants["group: only, 200 groups"] = lambda: rt.hamming_topk_filtered(q, g, k, group=group200, want=want_grp)
            med = interleaved(variants)
            lines.append(f"{Qn} x {G} x 64 bit, k = {k}:")
            for n in variants:
                lines.append(f"  {n:28s} {med[n]:10.1f} us ({med[n] / med['unfiltered']:.3f}x)")
            same = rt.hamming_topk_filtered(q, g, k, allow=bitmaps["every row"])
            plain = rt.hamming_topk(q, g, k)
            lines.append(f"  every row admitted == unfiltered, bit for bit: {bool(torch.equal(same[0], plain[0]) and torch.equal(same[1], plain[1]))}")
        # the post-filter of today: the unfiltered 128 hits, filtered on the host
        idx128 = rt.hamming_topk(q, g, 128)[0]
        for n, v in allows.items():
            if n == "every row":
                continue
            kept = (v[idx128.clamp_min(0)] & (idx128 >= 0)).sum(1)
            avail = int(v.sum())
            lines.append(f"  post-filter of the unfiltered k = 128 list, allow {n}: delivers " +
                         ", ".join(f"{100 * float((kept.clamp_max(kk).float() / min(kk, avail)).mean()):.1f} % of k = {kk}" for kk in (10, 128)) +
                         f" (queries with a full list: " + ", ".join(f"{100 * float((kept >= min(kk, avail)).float().mean()):.1f} % at k = {kk}" for kk in (10, 128)) + ")")

    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        this = _lib.load()
        for name, (res, args) in _lib.SIGNATURES.items():
            if hasattr(parent, name):
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, args

        def under(lib, fn):   # fn with `lib` as the loaded library: the same Python around both
            def run():
                _lib._lib = lib
                try:
                    return fn()
                finally:
                    _lib._lib = this
            return run

        def against_parent(head, calls):
            times = interleaved({f"{n}, {who}": under(lib, fn) for n, fn in calls.items() for who, lib in (("this", this), ("parent", parent))},
                                rounds=True)
            lines.append(head)
            for n in calls:
                mine_, theirs_ = times[f"{n}, this"], times[f"{n}, parent"]
                m_, p_, spread = statistics.median(mine_), statistics.median(theirs_), max(theirs_) - min(theirs_)
                lines.append(f"  {n:28s} {m_:10.1f} / {p_:10.1f} us ({m_ / p_:.3f}x)   parent's rounds {min(theirs_):.1f} .. {max(theirs_):.1f} "
                             f"(spread {spread:.1f})" + ("   <- above the parent by more than its spread" if m_ - p_ > spread else ""))

        lines += ["", "The entries of the parent, this build against the parent's library (the two taking turns): microseconds per call, this / "
                      "parent, and the parent's own spread over its rounds (max - min), the margin of the comparison"]
        for Qn, G in ((5794, 5994), (1024, 1_000_000)):
            q, g, mask = rand(Qn, 1), rand(G, 1), rand(Qn, 1)
            codes = torch.randn(Qn, 64, device="cuda", generator=gen)
            planes = rt.weight_planes(codes, 8)[0]
            q3, g3 = rt.pack_ternary(codes, 0.3), rt.pack_ternary(torch.randn(G, 64, device="cuda", generator=gen), 0.3)
            allow = rt.row_bitmap(torch.rand(G, device="cuda", generator=gen) < 0.5)
            for k in (10, 128):
                shards = [rt.hamming_topk(q, part, k, g_index_base=i * (G // 4)) for i, part in enumerate(g.split(G // 4)[:4])]
                idx_lists, dist_lists = torch.stack([s[0] for s in shards]), torch.stack([s[1] for s in shards])
                against_parent(f"{Qn} x {G} x 64 bit, k = {k}:", {
                    "hamming_topk": lambda: rt.hamming_topk(q, g, k),
                    "hamming_topk_masked": lambda: rt.hamming_topk_masked(q, g, mask, k),
                    "hamming_topk_weighted": lambda: rt.hamming_topk_weighted(q, planes, g, k),
                    "ternary_topk": lambda: rt.ternary_topk(q3, g3, 64, k),
                    "hamming_topk_filtered": lambda: rt.hamming_topk_filtered(q, g, k, allow=allow),
                    "..._filtered, masked": lambda: rt.hamming_topk_filtered(q, g, k, allow=allow, mask=mask),
                    "..._filtered, weighted": lambda: rt.hamming_topk_filtered(q, g, k, allow=allow, planes=planes),
                    "ternary_topk_filtered": lambda: rt.ternary_topk_filtered(q3, g3, 64, k, allow=allow),
                    "topk_merge, 4 shards": lambda: rt.topk_merge(idx_lists, dist_lists)})
        dq = rt.prepare_dense(torch.randn(5794, 64, device="cuda", generator=gen), "cosine")
        dg = rt.prepare_dense(torch.randn(5994, 64, device="cuda", generator=gen), "cosine")
        against_parent("dense, 5794 x 5994 x 64 dimensions, cosine, k = 10:", {"dense_topk": lambda: rt.dense_topk(dq, dg, "cosine", 10)})

text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
