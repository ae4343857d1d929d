"""GPU: the tie bracket -- ch_hamming_tie_bracket against the numpy closed form of tests/tie_bracket_ref.py bit
for bit, and the switch `tie_bracket` through retrieval.evaluate, the sharded evaluator (two gloo ranks on the one GPU), utils.hashing
and the evaluation command."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

LIMITS6 = [1, 5, 10, 100, 1000, -1]
LIMITS16 = [1, 2, 3, 5, 8, 10, 20, 50, 64, 65, 100, 200, 500, 1000, 2999, -1]
# Means of per-query ratios in [0, 1] are float64 sums whose order differs between the stable statistic (one column at a time) and the
# bracket (all columns at once): with at most a few hundred queries here the two roundings differ by < Qn * 2^-53 < 1e-13.
MEAN_EPS = 1e-13
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
    """packed codes around one random centre per class, every bit of a row flipped with probability `flip` (what trained codes look
    like: the buckets near a query are deep and relevant-heavy) -> (uint64 [rows, W], int32 labels)"""
    centres = np.random.default_rng(centre_seed).integers(0, 2, size=(nclass, 64 * W), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, nclass, size=rows).astype(np.int32)
    bits = centres[labels] ^ (rng.random((rows, 64 * W)) < flip).astype(np.uint8)
    packed = np.packbits(bits.reshape(rows, W, 64), axis=-1, bitorder="little").view(np.uint64).reshape(rows, W)
    return packed, labels


def _kernel_vs_ref(counts, limits, remove_first, dev):
    from concepthash_amd import retrieval as rt
    import tie_bracket_ref as tb
    uniq, _ = rt.normalize_limits(limits)
    got = [x.cpu().numpy() for x in rt.tie_bracket(_t(counts.astype(np.uint32), dev), uniq, remove_first)]
    torch.cuda.synchronize()
    want = tb.bracket_from_counts(counts, uniq, remove_first)
    for name, g_, w_ in zip(("S_low", "nrel_low", "S_high", "nrel_high"), got, want):
        assert np.array_equal(g_.view(w_.dtype), w_), (name, np.argwhere(g_.view(w_.dtype) != w_)[:5])
    return want


@pytest.mark.parametrize("remove_first", [False, True])
@pytest.mark.parametrize("W,limits", [(1, LIMITS6), (1, LIMITS16), (2, LIMITS6), (4, LIMITS16)])
def test_kernel_equals_closed_form_on_clustered_codes(dev, W, limits, remove_first):
    import tie_bracket_ref as tb
    q, ql = clustered(37, W, 6, 0.10, seed=1)            # 37 queries: not a multiple of the four waves of a workgroup
    g, gl = clustered(3000, W, 6, 0.10, seed=2)
    ql[5] = 6                                            # a query with no relevant row at all
    counts = tb.counts_from_codes(q, g, ql, gl)
    assert counts.shape == (37, 64 * W + 1, 2) and counts[5, :, 1].sum() == 0
    assert counts[:, :, 1].max() > 20                    # deep relevant-heavy buckets
    S_lo, n_lo, S_hi, n_hi = _kernel_vs_ref(counts, limits, remove_first, dev)
    assert (tb.ap_from_fixed(S_lo, n_lo) <= tb.ap_from_fixed(S_hi, n_hi)).all()
    assert (S_lo[:, 5] == 0).all() and (n_hi[:, 5] == 0).all()


@pytest.mark.parametrize("remove_first", [False, True])
def test_kernel_multi_hot_labels_and_one_row_gallery(dev, remove_first):
    import tie_bracket_ref as tb
    rng = np.random.default_rng(4)
    q, _ = clustered(21, 2, 5, 0.25, seed=5)
    g, _ = clustered(1500, 2, 5, 0.25, seed=6)
    qm, gm = (rng.random((21, 70)) < 0.03).astype(np.int8), (rng.random((1500, 70)) < 0.03).astype(np.int8)
    _kernel_vs_ref(tb.counts_from_codes(q, g, qm, gm), LIMITS6, remove_first, dev)
    for rel in (0, 1):                                   # a gallery of one row, relevant or not
        counts = np.zeros((3, 65, 2), dtype=np.uint32)
        counts[:, 17] = (1, rel)
        want = _kernel_vs_ref(counts, LIMITS6, remove_first, dev)
        assert (want[3] == (0 if remove_first else rel)).all()
    _kernel_vs_ref(np.zeros((2, 65, 2), dtype=np.uint32), [3, -1], remove_first, dev)      # no gallery row at all


@pytest.mark.parametrize("remove_first", [False, True])
def test_kernel_on_deep_mixed_buckets_cut_by_every_limit(dev, remove_first):
    """counts drawn directly: up to 300 rows per bucket with any share of relevant ones, so nearly every limit cuts a mixed bucket and
    the candidate search (every feasible number of relevant rows inside the limit) decides the result"""
    rng = np.random.default_rng(9)
    n = rng.integers(0, 301, size=(13, 65)) * (rng.random((13, 65)) < 0.5)
    r = (n * rng.random((13, 65))).astype(np.int64)
    counts = np.stack([n, r], axis=-1).astype(np.uint32)
    _kernel_vs_ref(counts, LIMITS16, remove_first, dev)
    _kernel_vs_ref(counts, [7, 77, 777, 7777], remove_first, dev)


@pytest.mark.parametrize("remove_first", [False, True])
def test_evaluate_with_the_switch(dev, remove_first):
    from concepthash_amd import retrieval as rt
    import tie_bracket_ref as tb
    q, ql = clustered(101, 1, 8, 0.25, seed=11)
    g, gl = clustered(4000, 1, 8, 0.25, seed=12)
    if remove_first:
        g[:101], gl[:101] = q, ql                       # the queries are part of the gallery
    R, ks = [10, 100, -1], (1, 5, 10)
    args = (_t(q, dev), _t(g, dev), _t(ql, dev), _t(gl, dev))
    off = rt.evaluate(*args, R=R, ks=ks, remove_first=remove_first)
    assert sorted(off) == KEYS_WITHOUT_THE_SWITCH
    rec = rt.evaluate(*args, R=R, ks=ks, remove_first=remove_first, records=True, tie_bracket=True)
    two = rt.evaluate(*args, R=R, ks=ks, remove_first=remove_first, records=False, tie_bracket=True)
    assert sorted(rec) == sorted(KEYS_WITHOUT_THE_SWITCH + list(rt.TIE_KEYS)) == sorted(two)
    counts = tb.counts_from_codes(q, g, ql, gl)
    want = tb.bracket_from_counts(counts, R, remove_first)
    for ev in (rec, two):
        for i in range(len(R)):
            # the stable statistics do not move with the switch
            assert torch.equal(ev["S"][i], off["S"][i]) and torch.equal(ev["nrel"][i], off["nrel"][i]) and ev["mAP"][i] == off["mAP"][i]
            for name, w_ in zip(("S_low", "nrel_low", "S_high", "nrel_high"), want):
                assert np.array_equal(ev[name][i].cpu().numpy().view(w_.dtype), w_[i]), (name, i)
            print(f"R={R[i]} remove_first={remove_first}: mAP {ev['mAP'][i]:.6f} in [{ev['mAP_low'][i]:.6f}, {ev['mAP_high'][i]:.6f}]")
            assert ev["mAP_low"][i] <= ev["mAP"][i] <= ev["mAP_high"][i]
            assert (ev["ap_low"][i] <= ev["ap"][i]).all() and (ev["ap"][i] <= ev["ap_high"][i]).all()
        assert ev["precisions"] == off["precisions"] and ev["recalls"] == off["recalls"] and torch.equal(ev["hits"], off["hits"])
        assert (ev["hits_low"] <= ev["hits"]).all() and (ev["hits"] <= ev["hits_high"]).all()
        ext = np.array([[tb.hits_extremes(counts[qi], k, remove_first) for k in ks] for qi in range(len(q))])   # [Qn, nk, 4]
        assert np.array_equal(ev["hits_low"].cpu().numpy(), ext[:, :, 0]) and np.array_equal(ev["hits_high"].cpu().numpy(), ext[:, :, 1])
        assert np.allclose(ev["precisions_low"], (ext[:, :, 0] / np.array(ks)).mean(0), atol=1e-14)
        assert np.allclose(ev["precisions_high"], (ext[:, :, 1] / np.array(ks)).mean(0), atol=1e-14)
        assert np.allclose(ev["recalls_low"], ext[:, :, 2].mean(0), atol=1e-14) and np.allclose(ev["recalls_high"], ext[:, :, 3].mean(0), atol=1e-14)
        for t in range(len(ks)):        # per query the integers nest exactly (above); the MEANS are float64 sums taken in different orders
            assert ev["precisions_low"][t] - MEAN_EPS <= ev["precisions"][t] <= ev["precisions_high"][t] + MEAN_EPS
            assert ev["recalls_low"][t] - MEAN_EPS <= ev["recalls"][t] <= ev["recalls_high"][t] + MEAN_EPS
    one = rt.evaluate(*args, R=100, ks=ks, remove_first=remove_first, tie_bracket=True)      # a single R: scalars, not lists
    assert one["mAP_low"] == rec["mAP_low"][1] and torch.equal(one["S_high"], rec["S_high"][1]) and isinstance(one["mAP_high"], float)
    empty = rt.evaluate(args[0], args[1][:0], args[2], args[3][:0], R=R, ks=ks, tie_bracket=True)
    assert sorted(empty) == sorted(rec) and empty["mAP_low"] == [0.0] * 3 and empty["precisions_high"] == [0.0] * 3


def test_the_mean_convention_reaches_the_bracket(dev):
    """R = 2 on one bucket {irr, irr, rel}: the pessimistic order has no relevant row inside R, the optimistic one has"""
    from concepthash_amd import retrieval as rt
    counts = np.zeros((3, 65, 2), dtype=np.uint32)
    counts[0, 4] = (3, 1)
    counts[1, 0] = (1, 1)
    counts[1, 9] = (5, 0)
    counts[2, 7] = (4, 0)
    c = _t(counts, dev)
    a = rt.tie_results(c, [2], [1], False, False, skip_queries_without_relevant=False)
    b = rt.tie_results(c, [2], [1], False, False, skip_queries_without_relevant=True)
    assert a["mAP_low"] == pytest.approx(1 / 3) and a["mAP_high"] == pytest.approx(2 / 3)
    assert b["mAP_low"] == 1.0 and b["mAP_high"] == 1.0
    assert a["nrel_low"].tolist() == [0, 1, 0] and a["nrel_high"].tolist() == [1, 1, 0]
    assert a["hits_low"][:, 0].tolist() == [0, 1, 0] and a["hits_high"][:, 0].tolist() == [1, 1, 0]


# ---- sharded: two gloo ranks sharing the one GPU (fresh child processes) ---------------------------------------------------------
def _problem():
    q, ql = clustered(61, 1, 6, 0.25, seed=21)
    g, gl = clustered(2500, 1, 6, 0.25, seed=22)
    return q, ql, g, gl


def _rank_main(rank, port, out_dir, remove_first):
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
        ev = sr.evaluate(_t(q, dev), _t(ql, dev), R=[10, 100, -1], ks=(1, 5, 10), remove_first=remove_first, tie_bracket=True)
        off = sr.evaluate(_t(q, dev), _t(ql, dev), R=[10, 100, -1], ks=(1, 5, 10), remove_first=remove_first)
        assert sorted(off) == KEYS_WITHOUT_THE_SWITCH
        torch.cuda.synchronize()
        _save(os.path.join(out_dir, f"r{rank}.npz"), ev, mAP_off=np.array(off["mAP"]))
    finally:
        dist.destroy_process_group()


FIELDS = ("S", "nrel", "S_low", "S_high", "nrel_low", "nrel_high")


def _save(path, ev, **extra):
    np.savez(path, **{k: torch.stack(ev[k]).cpu().numpy() for k in FIELDS}, hits_low=ev["hits_low"].cpu().numpy(),
             hits_high=ev["hits_high"].cpu().numpy(), mAP=np.array(ev["mAP"]), mAP_low=np.array(ev["mAP_low"]), mAP_high=np.array(ev["mAP_high"]),
             P_low=np.array(ev["precisions_low"]), R_high=np.array(ev["recalls_high"]), **extra)


def _single_main(out_dir, remove_first):
    """the same problem in ONE process (retrieval.evaluate): what the two ranks must reproduce"""
    sys.path.insert(0, ROOT)
    from concepthash_amd import retrieval as rt
    dev = torch.device("cuda:0")
    q, ql, g, gl = _problem()
    one = rt.evaluate(_t(q, dev), _t(g, dev), _t(ql, dev), _t(gl, dev), R=[10, 100, -1], ks=(1, 5, 10), remove_first=remove_first,
                      tie_bracket=True)
    torch.cuda.synchronize()
    _save(os.path.join(out_dir, "one.npz"), one)


@pytest.mark.parametrize("remove_first", [False, True])
def test_two_rank_sharded_bracket_equals_single_process(tmp_path, remove_first):
    """Every GPU step of this test runs in a fresh child process: the two ranks together, then (after they have ended) the
    single-process evaluation -- the test itself never touches the device, so it adds at most two processes with the GPU open."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    me = os.path.abspath(__file__)
    procs = [subprocess.Popen([sys.executable, me, "--rank", str(r), str(port), str(tmp_path), str(int(remove_first))], env=env)
             for r in range(2)]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    subprocess.run([sys.executable, me, "--single", str(tmp_path), str(int(remove_first))], env=env, check=True, timeout=300)
    one = np.load(tmp_path / "one.npz")
    assert (one["S_low"] != one["S_high"]).any()
    for r in range(2):
        z = np.load(tmp_path / f"r{r}.npz")
        for k in FIELDS + ("hits_low", "hits_high"):
            assert np.array_equal(z[k], one[k]), k
        assert z["mAP"].tolist() == one["mAP"].tolist() == z["mAP_off"].tolist()
        for k in ("mAP_low", "mAP_high", "P_low", "R_high"):
            assert z[k].tolist() == one[k].tolist(), k


# ---- surface -------------------------------------------------------------------------------------------------------------------
def test_calculate_map_keeps_its_triple_and_leaves_the_bracket_in_the_module(dev):
    from utils import hashing
    rng = np.random.default_rng(3)
    C, nbit = 11, 64
    centres = rng.standard_normal((C, nbit)).astype(np.float32)
    ql, gl = rng.integers(0, C, 150), rng.integers(0, C, 1200)
    qc = torch.from_numpy(centres[ql] + 0.9 * rng.standard_normal((150, nbit)).astype(np.float32))
    gc = torch.from_numpy(centres[gl] + 0.9 * rng.standard_normal((1200, nbit)).astype(np.float32))
    qoh, goh = torch.eye(C)[ql], torch.eye(C)[gl]
    plain = hashing.calculate_mAP(gc, goh, qc, qoh, [50, -1], PRs=[1, 5, 10])
    assert hashing.last_tie_bracket is None
    tied = hashing.calculate_mAP(gc, goh, qc, qoh, [50, -1], PRs=[1, 5, 10], tie_bracket=True)
    assert tied == plain and len(tied) == 3
    br = hashing.last_tie_bracket
    assert sorted(br) == ["mAP_high", "mAP_low", "precisions_high", "precisions_low", "recalls_high", "recalls_low"]
    for i in range(2):
        assert br["mAP_low"][i] <= plain[0][i] <= br["mAP_high"][i]
    assert br["mAP_low"][1] < br["mAP_high"][1]                         # 1,200 rows on 65 distances: ties exist
    for t in range(3):
        assert br["recalls_low"][t] - MEAN_EPS <= plain[1][t] <= br["recalls_high"][t] + MEAN_EPS
        assert br["precisions_low"][t] - MEAN_EPS <= plain[2][t] <= br["precisions_high"][t] + MEAN_EPS
    m, _, _ = hashing.calculate_mAP(gc, goh, qc, qoh, -1, PRs=[1], tie_bracket=True)
    assert isinstance(hashing.last_tie_bracket["mAP_low"], float) and hashing.last_tie_bracket["mAP_low"] <= m
    hashing.calculate_mAP(gc, goh, qc, qoh, -1, PRs=[1])
    assert hashing.last_tie_bracket is None


def test_evaluation_command_writes_the_bracket_only_when_asked(tmp_path):
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

    h0, out0 = run([], "ev0")
    assert not [k for k in h0 if "tie" in k] and "over tie orders" not in out0
    h1, out1 = run(["tie_bracket=true"], "ev1")
    assert f"mAP@-1: {h0['mAP'][1]:.4f}" in out0.splitlines() and f"mAP@-1: {h0['mAP'][1]:.4f}" in out1.splitlines()   # the evaluator's own lines stay
    assert h1["mAP"] == h0["mAP"] and h1["precisions"] == h0["precisions"] and h1["recalls"] == h0["recalls"]
    assert sorted(set(h1) - set(h0)) == ["mAP_tie_high", "mAP_tie_low"]
    for i in range(2):
        assert h1["mAP_tie_low"][i] <= h1["mAP"][i] <= h1["mAP_tie_high"][i]
    assert out1.count("over tie orders") == 2
    line = [ln for ln in out1.splitlines() if ln.startswith("mAP@-1:") and "tie" in ln][0]
    assert line == f"mAP@-1: {h1['mAP'][1]:.4f}  [{h1['mAP_tie_low'][1]:.4f}, {h1['mAP_tie_high'][1]:.4f}] over tie orders"


def test_training_command_records_the_bracket_only_when_asked(tmp_path):
    """`python main_v2.py exp=hashing ...` (experiments/train_helper.py): the evaluation step of a one-epoch run writes
    `mAP_tie_low` / `mAP_tie_high` into test_history.json with `tie_bracket=true`, and exactly the usual keys without it."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["dataset=synthetic_cub200", "dataset.limit=64", "dataset.nclass=8", "data_dir=" + str(tmp_path)]

    def run(extra, name):
        logdir = str(tmp_path / name)
        subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "exp=hashing", "optim=sgd", "optim.lr=0.02", "scheduler=no_decay",
                        "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64", "epochs=1", "eval_interval=1",
                        "batch_size=32", "logdir=" + logdir] + common + extra, check=True, env=env, cwd=str(tmp_path), timeout=600)
        te = json.load(open(os.path.join(logdir, "test_history.json")))
        assert len(te) == 1
        return te[0]

    off = run([], "run_off")
    assert not [k for k in off if "tie" in k] and 0.0 < off["mAP"] <= 1.0
    on = run(["tie_bracket=true"], "run_on")
    assert sorted(set(on) - set(off)) == ["mAP_tie_high", "mAP_tie_low"] and set(off) <= set(on)
    assert on["mAP"] == off["mAP"]                                     # seeded run: same codes, and the switch moves no stable number
    assert on["mAP_tie_low"] <= on["mAP"] <= on["mAP_tie_high"]


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--rank":
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], bool(int(sys.argv[5])))
elif __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--single":
    _single_main(sys.argv[2], bool(int(sys.argv[3])))
