"""GPU: the tie expectation -- ch_hamming_tie_expected against the exact references of tests/tie_expected_ref.py
within the bound derived there, and the switch `tie_expected` through retrieval.evaluate, the sharded evaluator (two gloo ranks on the
one GPU), utils.hashing and the evaluation and training commands.

Measured on one MI355X (each kernel test prints its figures): worst |kernel - exact| 2.2e-16 on the clustered problems (bounds up to
1.4e-14), 1.1e-16 on the edge shapes (3.4e-14), 3.3e-16 on the deep mixed buckets (3.5e-13), 2.2e-16 on the 2^31-row case (9.1e-12) and
2.2e-16 against the enumeration of tiny problems (allowed: 1e-12)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

LIMITS1 = [100]
LIMITS6 = [1, 5, 10, 100, 1000, -1]
LIMITS16 = [1, 2, 3, 5, 8, 10, 20, 50, 64, 65, 100, 200, 500, 1000, 2999, -1]
KS = (1, 5, 10, 100)
PROJECT_EPS = 1e-9        # |mAP_fixed - mAP_float64| of DESIGN.md section 2.0: every derived bound used here must stay under it
MEAN_EPS = 1e-13          # a mean of <= a few hundred per-query values in [0, 1], summed in another order: < Qn * 2^-53
KEYS_WITHOUT_THE_SWITCH = ["S", "ap", "hits", "mAP", "nrel", "precisions", "recalls", "total"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def clustered(rows, W, nclass, flip, seed, centre_seed=100):
    """packed codes around one random centre per class, every bit of a row flipped with probability `flip` -> (uint64 [rows, W], int32
    labels): the buckets near a query are deep and relevant-heavy"""
    centres = np.random.default_rng(centre_seed).integers(0, 2, size=(nclass, 64 * W), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, nclass, size=rows).astype(np.int32)
    bits = centres[labels] ^ (rng.random((rows, 64 * W)) < flip).astype(np.uint8)
    packed = np.packbits(bits.reshape(rows, W, 64), axis=-1, bitorder="little").view(np.uint64).reshape(rows, W)
    return packed, labels


def _kernel_vs_ref(counts, limits, ks, remove_first, dev, tol=None, ctx=None):
    """the kernel on `counts` against the reference (256-bit fixed point unless `ctx`), every query within its own derived bound (or within
    `tol`); -> (worst error, largest bound)"""
    from concepthash_amd import retrieval as rt
    import tie_expected_ref as te
    uniq, _ = rt.normalize_limits(limits)
    ap, hits, rec = (x.cpu().numpy() for x in rt.tie_expected(_t(counts.astype(np.uint32), dev), uniq, ks, remove_first))
    torch.cuda.synchronize()
    assert ap.shape == (len(uniq), len(counts)) and hits.shape == rec.shape == (len(ks), len(counts)) and ap.dtype == np.float64
    want_ap, want_h, want_r = te.expected_from_counts(counts, uniq, ks, remove_first, ctx)
    worst = top = 0.0
    for qi in range(len(counts)):
        b = [(int(n), int(r)) for n, r in counts[qi]]
        for li, R in enumerate(uniq):
            bound = te.error_bound(b, R, remove_first)
            assert bound < PROJECT_EPS
            err = abs(ap[li, qi] - want_ap[li][qi])
            worst, top = max(worst, err), max(top, bound)
            assert err <= (bound if tol is None else tol), (qi, R, remove_first, ap[li, qi], want_ap[li][qi], bound)
        for t, k in enumerate(ks):
            hb, rb = te.hits_bound(b, k, remove_first)
            assert abs(hits[t, qi] - want_h[t][qi]) <= hb and abs(rec[t, qi] - want_r[t][qi]) <= rb, (qi, k, hits[t, qi], want_h[t][qi])
    print(f"worst |kernel - exact| = {worst:.3g} under a bound of {top:.3g} ({len(counts)} queries, {len(uniq)} limits, "
          f"remove_first={remove_first})")
    return worst, top


@pytest.mark.parametrize("remove_first", [False, True])
@pytest.mark.parametrize("W,limits,Qn", [(1, LIMITS16, 64), (2, LIMITS6, 101), (4, LIMITS1, 64), (4, LIMITS16, 256)])
def test_kernel_within_the_derived_bound_on_clustered_codes(dev, W, limits, Qn, remove_first):
    import tie_bracket_ref as tb
    q, ql = clustered(Qn, W, 6, 0.10, seed=1)            # 101 queries: not a multiple of the four waves of a workgroup
    g, gl = clustered(3000, W, 6, 0.10, seed=2)
    ql[5] = 6                                            # a query with no relevant row at all
    counts = tb.counts_from_codes(q, g, ql, gl)
    assert counts[5, :, 1].sum() == 0 and counts[:, :, 0].max() > 100     # buckets of hundreds of rows, cut by the limits
    _kernel_vs_ref(counts, limits, KS, remove_first, dev)
    from concepthash_amd import retrieval as rt
    ap, hits, rec = rt.tie_expected(_t(counts, dev), [0], KS, remove_first)
    assert (ap[:, 5] == 0).all() and (hits[:, 5] == 0).all() and (rec[:, 5] == 0).all()


def edge_counts():
    """buckets drawn by hand (the limits of `EDGE_LIMITS` meet them as the comments say); one query per relevance pattern"""
    counts = np.zeros((6, 65, 2), dtype=np.uint32)
    # rows 1-5 | 6-45 without a relevant row | 46-75 all relevant | 76-175 mixed
    counts[0, 3], counts[0, 7], counts[0, 9], counts[0, 12] = (5, 2), (40, 0), (30, 30), (100, 37)
    counts[1] = counts[0]
    counts[1, :, 1] = 0                                  # no relevant row anywhere
    counts[2, 0], counts[2, 7], counts[2, 30] = (1, 1), (40, 0), (60, 0)      # remove_first drops the only relevant row
    counts[3, 64] = (1, 1)                               # a gallery of one row, relevant ...
    counts[4, 17] = (1, 0)                               # ... or not
    # query 5: no gallery row at all (an empty bucket list)
    return counts


# boundary of bucket 1 and one row either side; take = 1 and take = n - 1 in the r = 0 bucket; its end; take = 1 and n - 1 in the r = n
# bucket; its end and one past; inside the mixed bucket; its last row but one; G; G + 1; no limit
EDGE_LIMITS = [4, 5, 6, 44, 45, 46, 74, 75, 76, 100, 174, 175, 176, -1]


@pytest.mark.parametrize("remove_first", [False, True])
def test_kernel_on_edge_shapes_and_multi_hot_labels(dev, remove_first):
    import tie_bracket_ref as tb
    import tie_expected_ref as te
    from concepthash_amd import retrieval as rt
    counts = edge_counts()
    _kernel_vs_ref(counts, EDGE_LIMITS, (1, 5, 6, 45, 46, 176), remove_first, dev)
    _kernel_vs_ref(counts, [1], (1,), remove_first, dev)                 # one limit, one k
    ap, hits, rec = (x.cpu().numpy() for x in rt.tie_expected(_t(counts, dev), [0], (1, 200), remove_first))
    assert (ap[0, [1, 4, 5]] == 0).all() and (hits[:, [1, 4, 5]] == 0).all() and (rec[:, [1, 4, 5]] == 0).all()
    assert ap[0, 3] == (0.0 if remove_first else 1.0) and ap[0, 2] == (0.0 if remove_first else 1.0)
    assert rec[1, 2] == (0.0 if remove_first else 1.0)
    # exactly the Fractions on this small problem, too
    _kernel_vs_ref(counts[:1], EDGE_LIMITS, (), remove_first, dev, ctx=te.EXACT)
    rng = np.random.default_rng(4)
    q, _ = clustered(21, 2, 5, 0.25, seed=5)
    g, _ = clustered(1500, 2, 5, 0.25, seed=6)
    qm, gm = (rng.random((21, 70)) < 0.03).astype(np.int8), (rng.random((1500, 70)) < 0.03).astype(np.int8)
    _kernel_vs_ref(tb.counts_from_codes(q, g, qm, gm), LIMITS6, KS, remove_first, dev)


@pytest.mark.parametrize("remove_first", [False, True])
def test_kernel_on_deep_mixed_buckets_cut_by_every_limit(dev, remove_first):
    """counts drawn directly: up to 700 rows per bucket with any share of relevant ones, so nearly every limit cuts a mixed bucket and
    the weights run over several trips of 64"""
    rng = np.random.default_rng(9)
    n = rng.integers(0, 701, size=(64, 65)) * (rng.random((64, 65)) < 0.5)
    r = (n * rng.random((64, 65))).astype(np.int64)
    counts = np.stack([n, r], axis=-1).astype(np.uint32)
    _kernel_vs_ref(counts, [7, 77, 777, 3333, 7777, 9999, -1], KS, remove_first, dev)


def test_kernel_on_two_to_the_31_rows_in_one_bucket(dev):
    """built as counts, no codes: one bucket of about 2^31 rows, cut by limits that take 1 .. 8,191 of its rows -- few, half or nearly all
    of them relevant, with 1,000 or 2^31 rows ranked in front.  The reference is the 256-bit fixed point; nothing sums over the bucket."""
    counts = np.zeros((4, 65, 2), dtype=np.uint32)
    big = 2 ** 31 - 7
    counts[0, 5], counts[0, 9] = (1000, 400), (big, 2 ** 30 + 11)
    counts[1, 5], counts[1, 9] = (1000, 400), (big, 5000)
    counts[2, 5], counts[2, 9] = (1000, 0), (big, big - 3000)            # fewer irrelevant rows than `take`: tmin > 0
    counts[3, 2], counts[3, 6] = (big, 0), (2 ** 30, 2 ** 29)            # 2^31 rows ranked in front: the limits below do not reach the bucket
    limits = [1000, 1001, 1003, 4000, 5097, 9191]
    for remove_first in (False, True):
        worst, top = _kernel_vs_ref(counts[:3], limits, (1, 999, 1000, 3000, 9191), remove_first, dev)
        assert top < 1e-11
    far = [big, big + 1, big + 2500, big + 8191]
    _kernel_vs_ref(counts[3:], far, (big + 1, big + 8191), False, dev)


def test_kernel_equals_every_tie_order_of_tiny_problems(dev):
    """a handful of the problems tests/test_tie_expected_cpu.py enumerates, every R in 0 .. G + 1 (18 limits: two launches), within 1e-12"""
    import tie_expected_ref as te
    problems = [[(2, 1), (3, 2), (4, 2), (1, 0)], [(4, 2), (4, 2)], [(1, 1), (0, 0), (4, 3), (3, 0)], [(3, 3), (4, 1), (2, 2)],
                [(4, 0), (4, 4), (4, 2)], [(1, 0), (1, 1)], [(4, 1)]]
    counts = np.zeros((len(problems), 65, 2), dtype=np.uint32)
    for qi, b in enumerate(problems):
        for j, nr in enumerate(b):
            counts[qi, 3 + 7 * j] = nr
    from concepthash_amd import retrieval as rt
    limits = list(range(1, 18)) + [0]
    ks = (1, 2, 3, 5)
    worst = 0.0
    for rf in (False, True):
        ap, hits, rec = (x.cpu().numpy() for x in rt.tie_expected(_t(counts, dev), limits, ks, rf))
        for qi, b in enumerate(problems):
            w_ap, w_h, w_r = te.brute_force(b, limits, ks, rf)
            for li, R in enumerate(limits):
                worst = max(worst, abs(ap[li, qi] - float(w_ap[R])))
                assert abs(ap[li, qi] - float(w_ap[R])) <= 1e-12, (b, R, rf)
            for t, k in enumerate(ks):
                assert abs(hits[t, qi] - float(w_h[k])) <= 1e-12 and abs(rec[t, qi] - float(w_r[k])) <= 1e-12, (b, k, rf)
    print(f"worst |kernel - brute force| = {worst:.3g}")


def test_entry_refuses_bad_arguments(dev):
    from concepthash_amd import retrieval as rt
    c = torch.zeros(2, 65, 2, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="ascend"):
        rt.tie_expected(c, [10, 5])
    with pytest.raises(RuntimeError, match="nb = 64 W"):
        rt.tie_expected(torch.zeros(2, 300, 2, dtype=torch.int32, device=dev), [10])
    with pytest.raises(ValueError, match="k >= 1"):
        rt.tie_expected(c, [10], [0])
    with pytest.raises(TypeError):
        rt.tie_expected(c.to(torch.int64), [10])
    ap, hits, rec = rt.tie_expected(c[:0], [10], [1])
    assert ap.shape == (1, 0) and hits.shape == (1, 0)


# ---- the switch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remove_first", [False, True])
def test_evaluate_with_the_switch(dev, remove_first):
    from concepthash_amd import retrieval as rt
    import tie_bracket_ref as tb
    import tie_expected_ref as te
    q, ql = clustered(101, 1, 8, 0.25, seed=11)
    g, gl = clustered(4000, 1, 8, 0.25, seed=12)
    if remove_first:
        g[:101], gl[:101] = q, ql                       # the queries are part of the gallery
    R, ks = [10, 100, -1], (1, 5, 10)
    args = (_t(q, dev), _t(g, dev), _t(ql, dev), _t(gl, dev))
    off = rt.evaluate(*args, R=R, ks=ks, remove_first=remove_first)
    assert sorted(off) == KEYS_WITHOUT_THE_SWITCH
    on = rt.evaluate(*args, R=R, ks=ks, remove_first=remove_first, tie_expected=True)
    both = rt.evaluate(*args, R=R, ks=ks, remove_first=remove_first, tie_expected=True, tie_bracket=True)
    assert sorted(on) == sorted(KEYS_WITHOUT_THE_SWITCH + list(rt.EXPECTED_KEYS))
    assert sorted(both) == sorted(KEYS_WITHOUT_THE_SWITCH + list(rt.EXPECTED_KEYS) + list(rt.TIE_KEYS))
    for ev in (on, both):                               # every old key bit-identical
        for key in KEYS_WITHOUT_THE_SWITCH:
            a, b = ev[key], off[key]
            if isinstance(a, list) and isinstance(a[0], torch.Tensor):
                assert all(torch.equal(x, y) for x, y in zip(a, b)), key
            elif isinstance(a, torch.Tensor):
                assert torch.equal(a, b), key
            else:
                assert a == b, key
    for key in rt.EXPECTED_KEYS:                        # the same bits with and without the bracket beside it
        a, b = on[key], both[key]
        assert all(torch.equal(x, y) for x, y in zip(a, b)) if key == "ap_expected" else (torch.equal(a, b) if key == "hits_expected" else a == b)
    counts = tb.counts_from_codes(q, g, ql, gl)
    want_ap, want_h, want_r = te.expected_from_counts(counts[:24], [10, 100, 0], ks, remove_first)
    for i in range(3):
        print(f"R={R[i]} remove_first={remove_first}: mAP {both['mAP'][i]:.6f}, expected {both['mAP_expected'][i]:.6f} in "
              f"[{both['mAP_low'][i]:.6f}, {both['mAP_high'][i]:.6f}]")
        assert both["mAP_low"][i] - MEAN_EPS <= both["mAP_expected"][i] <= both["mAP_high"][i] + MEAN_EPS
        ae = both["ap_expected"][i]
        assert ae.dtype == torch.float64 and ae.shape == (101,)
        assert (both["ap_low"][i] - 1e-12 <= ae).all() and (ae <= both["ap_high"][i] + 1e-12).all()
        assert np.allclose(ae[:24].cpu().numpy(), want_ap[i], rtol=0, atol=1e-12)
        assert abs(both["mAP_expected"][i] - float(ae.mean())) <= MEAN_EPS
    he = both["hits_expected"]
    assert he.shape == (101, 3) and he.dtype == torch.float64
    assert (both["hits_low"] - 1e-12 <= he).all() and (he <= both["hits_high"] + 1e-12).all()
    assert np.allclose(he[:24].cpu().numpy().T, want_h, rtol=0, atol=1e-12)
    for t, k in enumerate(ks):
        assert abs(both["precisions_expected"][t] - float((he[:, t] / k).mean())) <= MEAN_EPS
        assert both["recalls_low"][t] - MEAN_EPS <= both["recalls_expected"][t] <= both["recalls_high"][t] + MEAN_EPS
    one = rt.evaluate(*args, R=100, ks=ks, remove_first=remove_first, tie_expected=True)      # a single R: scalars, not lists
    assert one["mAP_expected"] == on["mAP_expected"][1] and torch.equal(one["ap_expected"], on["ap_expected"][1])
    empty = rt.evaluate(args[0], args[1][:0], args[2], args[3][:0], R=R, ks=ks, tie_expected=True)
    assert sorted(empty) == sorted(on) and empty["mAP_expected"] == [0.0] * 3 and empty["hits_expected"].shape == (101, 3)
    with pytest.raises(ValueError, match="depends on the tie order"):
        rt.evaluate(*args, R=R, ks=ks, tie_expected=True, skip_queries_without_relevant=True)


# ---- sharded: two gloo ranks sharing the one GPU (fresh child processes) ---------------------------------------------------------------
def _problem():
    q, ql = clustered(61, 1, 6, 0.25, seed=21)
    g, gl = clustered(2500, 1, 6, 0.25, seed=22)
    return q, ql, g, gl


HOW = dict(R=[10, 100, -1], ks=(1, 5, 10))


def _save(path, ev, **extra):
    np.savez(path, S=torch.stack(ev["S"]).cpu().numpy(), ap_expected=torch.stack(ev["ap_expected"]).cpu().numpy(),
             hits_expected=ev["hits_expected"].cpu().numpy(), mAP=np.array(ev["mAP"]), mAP_expected=np.array(ev["mAP_expected"]),
             P_expected=np.array(ev["precisions_expected"]), R_expected=np.array(ev["recalls_expected"]), **extra)


def _rank_main(rank, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        from concepthash_amd.distributed import ShardedRetrieval
        dev = torch.device("cuda:0")
        q, ql, g, gl = _problem()
        lo, hi = [0, 900, 2500][rank], [0, 900, 2500][rank + 1]
        sr = ShardedRetrieval(_t(g[lo:hi], dev), _t(gl[lo:hi], dev))
        for remove_first in (False, True):
            ev = sr.evaluate(_t(q, dev), _t(ql, dev), remove_first=remove_first, tie_expected=True, **HOW)
            off = sr.evaluate(_t(q, dev), _t(ql, dev), remove_first=remove_first, **HOW)
            assert sorted(off) == KEYS_WITHOUT_THE_SWITCH
            torch.cuda.synchronize()
            _save(os.path.join(out_dir, f"r{rank}_{int(remove_first)}.npz"), ev, mAP_off=np.array(off["mAP"]))
        refused = False
        try:
            sr.evaluate(_t(q, dev), _t(ql, dev), tie_expected=True, skip_queries_without_relevant=True, **HOW)
        except ValueError:
            refused = True
        assert refused
    finally:
        dist.destroy_process_group()


def _single_main(out_dir):
    """the same problem in ONE process (retrieval.evaluate): what the two ranks must reproduce"""
    sys.path.insert(0, ROOT)
    from concepthash_amd import retrieval as rt
    dev = torch.device("cuda:0")
    q, ql, g, gl = _problem()
    for remove_first in (False, True):
        one = rt.evaluate(_t(q, dev), _t(g, dev), _t(ql, dev), _t(gl, dev), remove_first=remove_first, tie_expected=True, **HOW)
        torch.cuda.synchronize()
        _save(os.path.join(out_dir, f"one_{int(remove_first)}.npz"), one)


def test_two_rank_sharded_expectation_equals_single_process(tmp_path):
    """Every GPU step of this test runs in a fresh child process: the two ranks together, then (after they have ended) the
    single-process evaluation -- the test itself never touches the device, so it adds at most two processes with the GPU open.  Both
    processes evaluate with remove_first off and on."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    me = os.path.abspath(__file__)
    procs = [subprocess.Popen([sys.executable, me, "--rank", str(r), str(port), str(tmp_path)], env=env) for r in range(2)]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    subprocess.run([sys.executable, me, "--single", str(tmp_path)], env=env, check=True, timeout=300)
    for rf in (0, 1):
        one = np.load(tmp_path / f"one_{rf}.npz")
        assert (one["mAP_expected"] != one["mAP"]).any()
        for r in range(2):
            z = np.load(tmp_path / f"r{r}_{rf}.npz")
            for k in ("S", "ap_expected", "hits_expected"):
                assert np.array_equal(z[k], one[k]), (k, rf)
            assert z["mAP"].tolist() == one["mAP"].tolist() == z["mAP_off"].tolist()
            for k in ("mAP_expected", "P_expected", "R_expected"):
                assert z[k].tolist() == one[k].tolist(), (k, rf)


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_calculate_map_keeps_its_triple_and_leaves_the_expectation_in_the_module(dev):
    from utils import hashing
    rng = np.random.default_rng(3)
    C, nbit = 11, 64
    centres = rng.standard_normal((C, nbit)).astype(np.float32)
    ql, gl = rng.integers(0, C, 150), rng.integers(0, C, 1200)
    qc = torch.from_numpy(centres[ql] + 0.9 * rng.standard_normal((150, nbit)).astype(np.float32))
    gc = torch.from_numpy(centres[gl] + 0.9 * rng.standard_normal((1200, nbit)).astype(np.float32))
    qoh, goh = torch.eye(C)[ql], torch.eye(C)[gl]
    plain = hashing.calculate_mAP(gc, goh, qc, qoh, [50, -1], PRs=[1, 5, 10])
    assert hashing.last_tie_expected is None
    tied = hashing.calculate_mAP(gc, goh, qc, qoh, [50, -1], PRs=[1, 5, 10], tie_expected=True, tie_bracket=True)
    assert tied == plain and len(tied) == 3
    ex, br = hashing.last_tie_expected, hashing.last_tie_bracket
    assert sorted(ex) == ["mAP_expected", "precisions_expected", "recalls_expected"]
    for i in range(2):
        assert br["mAP_low"][i] - MEAN_EPS <= ex["mAP_expected"][i] <= br["mAP_high"][i] + MEAN_EPS
    assert br["mAP_low"][1] < ex["mAP_expected"][1] < br["mAP_high"][1]          # 1,200 rows on 65 distances: ties exist
    for t in range(3):
        assert br["precisions_low"][t] - MEAN_EPS <= ex["precisions_expected"][t] <= br["precisions_high"][t] + MEAN_EPS
        assert br["recalls_low"][t] - MEAN_EPS <= ex["recalls_expected"][t] <= br["recalls_high"][t] + MEAN_EPS
    m, _, _ = hashing.calculate_mAP(gc, goh, qc, qoh, -1, PRs=[1], tie_expected=True)
    assert isinstance(hashing.last_tie_expected["mAP_expected"], float) and hashing.last_tie_bracket is None
    hashing.calculate_mAP(gc, goh, qc, qoh, -1, PRs=[1])
    assert hashing.last_tie_expected is None


def test_evaluation_command_writes_the_expectation_only_when_asked(tmp_path):
    logdir = str(tmp_path / "run")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["dataset=synthetic_cub200", "dataset.limit=96", "data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True, env=env,
                   cwd=str(tmp_path), timeout=600)

    def run(extra, name):
        ev = str(tmp_path / name)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "--config-name", "val.yaml", "logdir=" + logdir,
                            "batch_size=32", "R=[10,-1]", "eval_logdir=" + ev] + common + extra, check=True, env=env, cwd=str(tmp_path),
                           timeout=600, capture_output=True, text=True)
        return json.load(open(os.path.join(ev, "history.json"))), r.stdout

    h0, out0 = run(["concept_eval=true"], "ev0")
    assert not [k for k in h0 if "expected" in k] and "expected" not in out0
    h1, out1 = run(["concept_eval=true", "tie_expected=true", "tie_bracket=true"], "ev1")
    assert h1["mAP"] == h0["mAP"] and h1["precisions"] == h0["precisions"] and h1["recalls"] == h0["recalls"]
    assert h1["mAP_concept"] == h0["mAP_concept"]
    assert sorted(set(h1) - set(h0)) == ["mAP_concept_expected", "mAP_expected", "mAP_tie_high", "mAP_tie_low", "precisions_expected",
                                         "recalls_expected"]
    for i in range(2):
        assert h1["mAP_tie_low"][i] - MEAN_EPS <= h1["mAP_expected"][i] <= h1["mAP_tie_high"][i] + MEAN_EPS
    assert len(h1["precisions_expected"]) == len(h1["precisions"]) and len(h1["recalls_expected"]) == len(h1["recalls"])
    assert len(h1["mAP_concept_expected"]) == len(h1["mAP_concept"]) and all(len(m) == 2 and 0.0 <= min(m) <= max(m) <= 1.0
                                                                            for m in h1["mAP_concept_expected"])
    line = [ln for ln in out1.splitlines() if ln.startswith("mAP@-1:") and "expected" in ln][-1]
    assert line == f"mAP@-1: {h1['mAP'][1]:.4f}  expected {h1['mAP_expected'][1]:.4f} over tie orders"


def test_training_command_records_the_expectation_when_asked(tmp_path):
    """`python main_v2.py exp=hashing ...` (experiments/train_helper.py): the evaluation step of a one-epoch run writes `mAP_tie_expected`
    into test_history.json with `tie_expected=true` -- alone: no bracket was asked for, none is written.  The run WITHOUT the keys is the first run of
    tests/test_tie_bracket_gpu.py::test_training_command_records_the_bracket_only_when_asked, which asserts that no key of it contains
    "tie": it is not repeated here."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    logdir = str(tmp_path / "run_on")
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "exp=hashing", "optim=sgd", "optim.lr=0.02", "scheduler=no_decay",
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64", "epochs=1", "eval_interval=1", "batch_size=32",
                    "logdir=" + logdir, "dataset=synthetic_cub200", "dataset.limit=64", "dataset.nclass=8", "data_dir=" + str(tmp_path),
                    "tie_expected=true"], check=True, env=env, cwd=str(tmp_path), timeout=600)
    te = json.load(open(os.path.join(logdir, "test_history.json")))
    assert len(te) == 1
    on = te[0]
    assert sorted(k for k in on if "tie" in k or "expected" in k) == ["mAP_tie_expected"] and 0.0 < on["mAP"] <= 1.0
    assert 0.0 < on["mAP_tie_expected"] <= 1.0


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--rank":
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
elif __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--single":
    _single_main(sys.argv[2])
