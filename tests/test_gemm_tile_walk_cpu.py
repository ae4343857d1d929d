"""csrc/gemm_tile_walk.h on the CPU: the one map from a GEMM launch's block id to its output tile (XCD remap, n-groups of group_n, the
partial last group, rev), which every bf16 GEMM kernel calls.  A stand-alone program (tests/gemm_tile_walk_test.cpp, the header alone,
g++ -fsanitize=undefined, run as a child process, no preload) walks every grid of the sweep; here every grid is checked to be a bijection
onto its tiles and to be, block by block, the order of the expression the kernels carried before the header existed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_M, MAX_N = 40, 12


def parent_order(bid, tiles_m, tiles_n, group_n, rev):
    """the lines every kernel had after `const int wg = xcd_remap(blockIdx.x, tiles_m * tiles_n);`, on an array of block ids"""
    nwg = tiles_m * tiles_n
    q, r, xcd, local = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    wg = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + local
    per_group = tiles_m * group_n
    g = wg // per_group
    rem = wg - g * per_group
    gn = np.minimum(group_n, tiles_n - g * group_n)
    tm_fwd = rem // gn
    tn = g * group_n + (rem - tm_fwd * gn)
    tm = tiles_m - 1 - tm_fwd if rev else tm_fwd
    return tm, tn


def test_tile_walk_is_a_bijection_in_the_parent_order(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "gemm_tile_walk_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "concepthash_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_tile_walk_test.cpp"), "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(MAX_M), str(MAX_N)], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
    pairs = np.frombuffer(r.stdout, dtype=np.int32).reshape(-1, 2)
    at = cases = 0
    for tiles_m in range(1, MAX_M + 1):
        for tiles_n in range(1, MAX_N + 1):
            tiles = tiles_m * tiles_n
            bid = np.arange(tiles, dtype=np.int64)
            for group_n in range(1, tiles_n + 1):
                for rev in (0, 1):
                    what = f"tiles_m {tiles_m} tiles_n {tiles_n} group_n {group_n} rev {rev}"
                    tm, tn = pairs[at:at + tiles, 0], pairs[at:at + tiles, 1]
                    assert len(tm) == tiles, what + ": the program wrote too few pairs"
                    assert tm.min() >= 0 and tm.max() < tiles_m and tn.min() >= 0 and tn.max() < tiles_n, what + ": a tile outside the grid"
                    hits = np.bincount(tm.astype(np.int64) * tiles_n + tn, minlength=tiles)
                    assert len(hits) == tiles and (hits == 1).all(), what + ": a tile is skipped or taken twice"
                    em, en = parent_order(bid, tiles_m, tiles_n, group_n, rev)
                    assert np.array_equal(tm, em) and np.array_equal(tn, en), what + ": not the parent's order"
                    at += tiles
                    cases += 1
    assert cases == 6240 and at == len(pairs)
