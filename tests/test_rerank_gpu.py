"""GPU: the two-stage search ("two-stage"; ch_dense_rerank in csrc/dense_rank.hip) -- a Hamming shortlist of the
sign codes ordered by a dense distance of the real-valued codes -- against the numpy reference of tests/rerank_ref.py.  Codes on the
grid where every fp32 operation is exact (multiples of 1/16 in [-4, 4]) are held to the reference bit for bit; gaussian codes are held
to the bits of `dense_dist` and to the shortlist of `hamming_ranked`, the passes that were there before."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import asymmetric_eval_ref as aref
import dense_ref as dref
import rerank_ref as rr
from conftest import ROOT

pytestmark = pytest.mark.gpu

G = 700
KS = (1, 5, 10)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _same_lists(got, want):
    """indices equal, distances equal bit for bit"""
    return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(dref.bits(got[1].cpu().numpy()), dref.bits(want[1]))


_GRID = {}


def _grid_problem(n, Qn=17):
    """Clustered grid codes: 5 class centres of signs, 40 distinct gallery rows (a centre's signs with a tenth flipped, times grid
    magnitudes), each drawn about 17 times into the 700 gallery rows -- so equal D abounds and every Hamming bucket holds copies, which
    the m-th place cuts through -- and queries drawn from the same centres.  -> (xq, xg, shortlist-independent labels)"""
    if (n, Qn) not in _GRID:
        rng = np.random.default_rng(600 + n)
        centres = np.where(rng.random((5, n)) < 0.5, -1.0, 1.0)

        def rows(count):
            lab = rng.integers(0, 5, count)
            sign = centres[lab] * np.where(rng.random((count, n)) < 0.1, -1.0, 1.0)
            return (sign * rng.integers(1, 65, (count, n)) / 16.0).astype(np.float32), lab
        distinct, dlab = rows(40)
        pick = rng.integers(0, 40, G)
        xq, ql = rows(Qn)
        _GRID[(n, Qn)] = (xq, distinct[pick], ql, dlab[pick])
    return _GRID[(n, Qn)]


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 48, 256])
@pytest.mark.parametrize("metric", ["dot", "euclidean"])
def test_two_stage_list_equals_the_reference_on_the_exact_grid(dev, metric, n):
    from concepthash_amd import retrieval as rt
    for Qn in (1, 17):
        xq, xg, _, _ = _grid_problem(n, Qn)
        D = dref.dist(xq, xg, metric)
        assert np.array_equal(D.astype(np.float32).astype(np.float64), D)   # the grid's distances are fp32 numbers
        srt = np.sort(D, 1)
        assert int((srt[:, 1:] == srt[:, :-1]).sum()) > 300 * Qn            # the index tie-break does real work
        ham = np.sort(dref.hamming(xq, xg), 1)
        tq, tg = _t(xq, dev), _t(xg, dev)
        for m in (1, 7, 256, 257, 1000, 4096):
            if 1 < m < G:
                assert (ham[:, m - 1] == ham[:, m]).any(), m                # the m-th place cuts through a Hamming tie bucket
            cand = rr.shortlist(xq, xg, m)
            for k in sorted({1, min(128, m), m}):
                got = rt.rerank_topk(tq, tg, metric, k, m)
                assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (Qn, k)
                assert _same_lists(got, rr.rerank(D, cand, k)), (Qn, m, k)
            if m >= G:                                                      # ... which is then the exhaustive list
                assert _same_lists(rt.rerank_topk(tq, tg, metric, 128, m), dref.topk(D, 128))
            else:                                                           # the same set as the Hamming list
                idx = rt.rerank_topk(tq, tg, metric, m, m)[0].cpu().numpy()
                assert np.array_equal(np.sort(idx, 1), np.sort(rt.hamming_ranked(rt.pack_sign(tq), rt.pack_sign(tg), m)[0].cpu().numpy(), 1))


# ---- gaussian codes: the bits of dense_dist, the shortlist of hamming_ranked ---------------------------------------------------------
@pytest.mark.parametrize("n", [30, 48, 64, 256])                            # 30: rows that are not 16-byte aligned (scalar loads)
@pytest.mark.parametrize("metric", dref.METRICS)
def test_rerank_ranks_by_the_bits_of_dense_dist(dev, metric, n):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(700 + n)
    Qn = 37
    xq, xg = rng.standard_normal((Qn, n)).astype(np.float32), rng.standard_normal((G, n)).astype(np.float32)
    xg[11] = 0.0                                                            # a zero row: cosine distance 1
    tq, tg = _t(xq, dev), _t(xg, dev)
    M = rt.dense_dist(rt.prepare_dense(tq, metric), rt.prepare_dense(tg, metric), metric).cpu().numpy()
    if metric == "cosine":
        assert np.all(M[:, 11] == 1.0)
    pq, pg = rt.pack_sign(tq), rt.pack_sign(tg)
    near = int(np.median(np.sort(dref.hamming(xq, xg), 1)[:, 200]))         # about 200 rows of a query lie within this many bits
    for m, radius in ((300, None), (257, near), (1000, None)):              # the radius leaves ragged shortlists
        cand, _ = rt.hamming_ranked(pq, pg, m, radius=radius)
        filled = (cand >= 0).sum(1).cpu().numpy()
        if radius is not None:
            assert filled.min() < filled.max() and filled.min() < m
        idx, dist = rt.dense_rerank(tq, tg, cand, metric, m)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        assert np.array_equal((idx >= 0).sum(1), filled) and np.all(idx[np.arange(m)[None, :] >= filled[:, None]] == -1)
        assert np.all(np.isposinf(dist[idx < 0]))
        live = idx >= 0
        assert np.array_equal(dref.bits(dist[live]), dref.bits(np.take_along_axis(M, np.maximum(idx, 0), 1)[live]))
        assert np.array_equal(idx, rr.rerank(M.astype(np.float64), cand.cpu().numpy(), m)[0])   # the lexsort of those bits over the shortlist
        assert _same_lists(rt.rerank_topk(tq, tg, metric, 10, m, radius=radius), (idx[:, :10], dist[:, :10]))
    # m >= G, k <= 128: the exhaustive list, idx and dist bits
    for k in (10, 128):
        full = rt.dense_topk(rt.prepare_dense(tq, metric), rt.prepare_dense(tg, metric), metric, k)
        two = rt.rerank_topk(tq, tg, metric, k, 1000)
        assert torch.equal(two[0], full[0]) and torch.equal(two[1].view(torch.int32), full[1].view(torch.int32))


@pytest.mark.parametrize("metric", dref.METRICS)
def test_hand_made_candidate_lists(dev, metric):
    """-1 in the middle, a row listed twice, a row past the gallery under validate=False, a base, a zero row, an empty list"""
    from concepthash_amd import retrieval as rt
    xq, xg, _, _ = _grid_problem(48)
    xq, xg = xq[:3].copy(), xg[:50].copy()
    xg[4] = 0.0
    xq[2] = 0.0
    tq, tg = _t(xq, dev), _t(xg, dev)
    M = rt.dense_dist(rt.prepare_dense(tq, metric), rt.prepare_dense(tg, metric), metric).cpu().numpy().astype(np.float64)
    cand = np.array([[7, -1, 4, 7, 49, -1, 0, 33, -5], [-1] * 9, [4, 3, 2, 1, 0, -1, 1, 1, 9]], np.int64)
    for base in (0, 1000):
        shifted = np.where(cand >= 0, cand + base, cand)
        for k in (1, 6, 9):
            got = rt.dense_rerank(tq, tg, _t(shifted, dev), metric, k, g_index_base=base)
            assert _same_lists(got, rr.rerank(M, shifted, k, base)), (base, k)
    idx, dist = rt.dense_rerank(tq, tg, _t(cand, dev), metric, 9)
    assert idx[1].tolist() == [-1] * 9 and bool(torch.isposinf(dist[1]).all())
    assert sorted(idx[0].tolist()) == [-1, -1, -1, 0, 4, 7, 7, 33, 49] and idx[2].tolist().count(1) == 3
    if metric == "cosine":
        assert float(dist[0][idx[0] == 4]) == 1.0 and dist[2, :7].tolist() == [1.0] * 7     # a zero row on either side
    # an id >= G: a ValueError from the wrapper, nothing launched; the kernel itself treats it as an empty slot
    over = cand.copy()
    over[0, 1] = 50
    with pytest.raises(ValueError, match="outside the gallery"):
        rt.dense_rerank(tq, tg, _t(over, dev), metric, 9)
    assert _same_lists(rt.dense_rerank(tq, tg, _t(over, dev), metric, 9, validate=False), rr.rerank(M, cand, 9))
    with pytest.raises(RuntimeError, match="1 <= k <= m <= 4096"):         # the entry's own status and message
        from concepthash_amd import _lib
        lib = _lib.load()
        _lib.check(lib.ch_dense_rerank(_lib.ptr(tq), 3, _lib.ptr(tg), 50, 48, 0, _lib.ptr(_t(cand, dev)), 9, 10, 0, None, None, None), "ch_dense_rerank")


# ---- the evaluation ----------------------------------------------------------------------------------------------------------------
def _labels(rng, ql, gl, multi, C=5):
    if not multi:
        q_lab = ql.copy()
        q_lab[3] = C                                                        # a class the gallery does not hold
        return q_lab, gl.copy()
    q_lab, g_lab = np.eye(C, dtype=np.int64)[ql], np.eye(C, dtype=np.int64)[gl]
    g_lab[rng.random(g_lab.shape) < 0.1] = 1
    q_lab[rng.random(q_lab.shape) < 0.1] = 1
    q_lab[3] = 0                                                            # no class at all
    return q_lab, g_lab


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
@pytest.mark.parametrize("multi", [False, True])
def test_evaluate_reranked_equals_the_brute_force_on_the_exact_grid(dev, metric, multi):
    from concepthash_amd import retrieval as rt
    xq, xg, ql, gl = _grid_problem(48)
    q_lab, g_lab = _labels(np.random.default_rng(800 + multi), ql, gl, multi)
    rel = aref.relevance(q_lab, g_lab)
    D = dref.dist(xq, xg, metric)
    tq, tg, tql, tgl = _t(xq, dev), _t(xg, dev), _t(q_lab, dev), _t(g_lab, dev)
    for m in (60, 1000):
        cand = rr.shortlist(xq, xg, m)
        for rf in (False, True):
            Rs = [-1, 50, 7]
            out = rt.evaluate_reranked(tq, tg, tql, tgl, metric, m, R=Rs, ks=KS, remove_first=rf)
            S, nrel, total = rr.evaluate(D, cand, rel, [m, 50, 7] + list(KS), rf)
            assert out["R"] == [m, 50, 7] and out["shortlist"] == m and isinstance(out["mAP"], list)
            for i in range(3):
                assert np.array_equal(out["S"][i].cpu().numpy().view(np.uint64), S[i]), (m, rf, i)
                assert np.array_equal(out["nrel"][i].cpu().numpy(), nrel[i]), (m, rf, i)
                ap = np.where(nrel[i] > 0, S[i].astype(np.float64) / (np.maximum(nrel[i], 1) * 2.0 ** 32), 0.0)
                assert out["mAP"][i] == pytest.approx(float(ap.mean()), abs=1e-12)
            assert np.array_equal(out["hits"].cpu().numpy(), nrel[3:].T) and np.array_equal(out["total"].cpu().numpy(), total)
            assert out["precisions"] == pytest.approx([float((nrel[3 + t] / k).mean()) for t, k in enumerate(KS)], abs=1e-12)
            assert out["recalls"] == pytest.approx([float(np.where(total > 0, nrel[3 + t] / np.maximum(total, 1), 0.0).mean()) for t in range(3)],
                                                   abs=1e-12)
            one = rt.evaluate_reranked(tq, tg, tql, tgl, metric, m, R=-1, ks=KS, remove_first=rf)
            assert one["mAP"] == out["mAP"][0] and one["R"] == m and torch.equal(one["S"], out["S"][0])
            # agreement with the exhaustive list: from the reference's own lists; 1.0 once the shortlist is the gallery
            full, two = dref.topk(D, 10)[0], rr.rerank(D, cand, 10)[0]
            assert out["agreement"] == pytest.approx({k: rr.agreement(full, two, k) for k in KS}, abs=1e-12)
            if m >= G:
                assert out["agreement"] == {k: 1.0 for k in KS}
    wide = rt.evaluate_reranked(tq, tg, tql, tgl, metric, 300, R=300, ks=[1, 200])
    assert list(wide["agreement"]) == [1]                                   # reported for k <= 128 only
    skipped = rt.evaluate_reranked(tq, tg, tql, tgl, metric, 60, R=-1, ks=[], skip_queries_without_relevant=True)
    plain = rt.evaluate_reranked(tq, tg, tql, tgl, metric, 60, R=-1, ks=[])
    has = int((plain["nrel"] > 0).sum())
    assert 0 < has < 17 and skipped["mAP"] == pytest.approx(plain["mAP"] * 17 / has, abs=1e-12)


# ---- surfaces ----------------------------------------------------------------------------------------------------------------------
def test_gallery_index_search_with_a_shortlist_returns_the_rows_of_rerank_topk(dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    from utils import hashing
    rng = np.random.default_rng(900)
    centres = np.where(rng.random((7, 64)) < 0.5, -1.0, 1.0)
    gl, ql = rng.integers(0, 7, G), rng.integers(0, 7, 37)
    xq, xg = aref.clustered_codes(rng, 37, 64, ql, centres), aref.clustered_codes(rng, G, 64, gl, centres)
    gt = _t(xg, dev)
    mean = gt.mean(0)
    index = GalleryIndex(rt.pack_sign(gt - mean), 64, 4, labels=_t(gl, dev), mean=mean, real=gt - mean)
    tq = _t(xq, dev) - mean
    for rank in dref.METRICS:
        for k, m, radius in ((10, 100, None), (300, 500, None), (20, 200, 8)):
            res = index.search(torch.from_numpy(xq), k, rank=rank, shortlist=m, radius=radius)
            idx, dist = rt.rerank_topk(tq, gt - mean, rank, k, m, radius=radius)
            assert torch.equal(res["idx"], idx) and torch.equal(res["dist"].view(torch.int32), dist.view(torch.int32))
            assert res["shortlist"] == m and res["rank"] == rank and res["dist"].dtype == torch.float32
            assert torch.equal(res["labels"], _t(gl, dev)[idx.clamp_min(0)].masked_fill(idx < 0, -1))
            assert res["concept_dist"].shape == (37, k, 4) and res["bits"].tolist() == [64] * 37
            if radius is not None:
                ham = dref.hamming(xq - mean.cpu().numpy(), xg - mean.cpu().numpy())
                inside = (ham <= radius).sum(1)
                assert np.array_equal((idx >= 0).sum(1).cpu().numpy(), np.minimum(inside, k)) and (inside < k).any()
    plain = index.search(torch.from_numpy(xq), 10, rank="cosine")          # without a shortlist: the exhaustive scan, as before
    assert "shortlist" not in plain
    assert torch.equal(plain["idx"], rt.dense_topk(rt.prepare_dense(tq, "cosine"), rt.prepare_dense(gt - mean, "cosine"), "cosine", 10)[0])
    # calculate_mAP(rank=<dense>, shortlist=m) is evaluate_reranked
    qoh, goh = torch.eye(7)[ql], torch.eye(7)[gl]
    want = rt.evaluate_reranked(_t(xq, dev), gt, _t(ql, dev), _t(gl, dev), "cosine", 100, R=-1, ks=KS, remove_first=True)
    got = hashing.calculate_mAP(torch.from_numpy(xg), goh, torch.from_numpy(xq), qoh, -1, PRs=list(KS), rank="cosine", shortlist=100,
                                remove_first_retrieved=True)
    assert got == (want["mAP"], want["recalls"], want["precisions"])
    assert hashing.last_rerank == dict(metric="cosine", shortlist=100, R=100, agreement=want["agreement"])
    assert 0.0 < want["agreement"][10] <= 1.0 and want["mAP"] > 0.3


COMMON = ["dataset=synthetic_cub200", "dataset.limit=96", "batch_size=32"]


def _main_v2(args, cwd):
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py")] + args, check=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=cwd,
                   timeout=600)


def test_the_search_and_the_validation_commands_with_a_shortlist(tmp_path, dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    logdir = str(tmp_path / "run")
    common = COMMON + ["data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), timeout=600)
    ev, s1 = str(tmp_path / "ev"), str(tmp_path / "s1")
    _main_v2(["--config-name", "val.yaml", "logdir=" + logdir, "save_code=True", "rerank_eval=true", "rerank_metric=cosine",
              "rerank_shortlist=50", "eval_logdir=" + ev] + common, str(tmp_path))
    outs = torch.load(os.path.join(ev, "outputs.pth"))
    te, db = outs["test"], outs["db"]
    gt = db["codes"].to(dev, torch.float32)
    hist = json.load(open(os.path.join(ev, "history.json")))
    want = rt.evaluate_reranked(te["codes"].to(dev), gt, te["labels"].to(dev), db["labels"].to(dev), "cosine", 50, R=-1, ks=(1, 5, 10))
    assert hist["mAP_rerank"] == want["mAP"] and hist["recalls_rerank"] == want["recalls"] and hist["precisions_rerank"] == want["precisions"]
    assert hist["rerank_metric"] == "cosine" and hist["rerank_shortlist"] == 50 and hist["rerank_R"] == 50
    assert hist["rerank_agreement"] == {str(k): v for k, v in want["agreement"].items()} and set(hist["rerank_agreement"]) == {"1", "5", "10"}
    assert "mAP" in hist and "mAP_dense" not in hist
    # exp=search rank=cosine shortlist=50 k=20: the index is built with the real plane, the only plane the search needs
    _main_v2(["--config-name", "search.yaml", "logdir=" + logdir, "search_logdir=" + s1, "rank=cosine", "shortlist=50", "k=20"] + common,
             str(tmp_path))
    res = json.load(open(os.path.join(s1, "results.json")))
    assert res["rank"] == "cosine" and res["k"] == 20 and res["shortlist"] == 50 and res["radius"] is None and res["index_rows"] == 96
    saved = GalleryIndex.load(os.path.join(logdir, "index_best.pth"))
    assert saved.real is not None and saved.mask is None and torch.equal(saved.real, gt.cpu())
    idx, dist = rt.rerank_topk(te["codes"].to(dev, torch.float32), gt, "cosine", 20, 50)
    idx, dist = idx.tolist(), dist.tolist()
    assert len(res["queries"]) == 96
    for i, e in enumerate(res["queries"]):
        assert [h["index"] for h in e["hits"]] == idx[i] and [h["distance"] for h in e["hits"]] == dist[i], i
