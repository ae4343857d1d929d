"""GPU: the rankings of real-valued codes (csrc/dense_rank.hip) -- ch_dense_prepare, ch_dense_dist, ch_dense_topk
and the rank-counting evaluation under the cosine, squared Euclidean and dot distances against the fp64 reference of tests/dense_ref.py,
at the smallest shapes that reach every path of the kernels.  Three kinds of input: codes on a grid where every fp32 operation is exact
in any order (multiples of 1/16 in [-4, 4]) and +-1 codes, where every comparison is exact, and gaussian codes, where the kernels are
held to the derived bounds of dense_ref and -- between their own passes -- to identical bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import asymmetric_eval_ref as aref
import dense_ref as dref
from conftest import ROOT

pytestmark = pytest.mark.gpu

QN, G = 37, 700
G_SEG, QN_SEG = 771, 70   # 256-row segments: three whole ones and a 3-row tail; five query tiles, the last with 6 of 16 queries
KS = (1, 5, 10)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _grid(rng, rows, n):
    """multiples of 1/16 in [-4, 4]: products, differences, squares and their sums over n <= 256 terms are exact in fp32"""
    return (rng.integers(-64, 65, (rows, n)) / 16.0).astype(np.float32)


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _same_lists(got, want):
    """indices equal, distances equal bit for bit"""
    return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(dref.bits(got[1].cpu().numpy()), dref.bits(want[1]))


def _labels(rng, multi, C=7, qn=QN, g=G):
    gl, ql = rng.integers(0, C, g), rng.integers(0, C, qn)
    if multi:
        q_lab, g_lab = np.eye(C, dtype=np.int64)[ql], np.eye(C, dtype=np.int64)[gl]
        g_lab[rng.random((g, C)) < 0.1] = 1
        q_lab[rng.random((qn, C)) < 0.1] = 1
        q_lab[3] = 0                                                    # no class at all: no relevant row
    else:
        q_lab, g_lab = ql.copy(), gl.copy()
        q_lab[3] = C                                                    # a class the gallery does not hold
    return q_lab, g_lab


def _check_eval(out, want, where=None):
    S, nrel, total = want                                               # limits were [R] + KS
    assert np.array_equal(out["S"].cpu().numpy().view(np.uint64), S[0]), where
    assert np.array_equal(out["nrel"].cpu().numpy(), nrel[0]) and np.array_equal(out["total"].cpu().numpy(), total), where
    assert np.array_equal(out["hits"].cpu().numpy(), nrel[1:].T), where


# ---- exact inputs: the distance matrix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 48, 120, 256])
@pytest.mark.parametrize("metric", ["dot", "euclidean"])
def test_dense_dist_equals_fp64_bit_for_bit_on_the_exact_grid(dev, n, metric):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(100 + n)
    xq, xg = _grid(rng, 9, n), _grid(rng, 131, n)
    xg[5] = 0.0
    xg[7] = xq[2]                                                       # euclidean 0; the most negative dot of query 2 with itself
    D = dref.dist(xq, xg, metric)
    assert np.array_equal(D.astype(np.float32).astype(np.float64), D)   # the grid's distances are fp32 numbers
    q, g = rt.prepare_dense(_t(xq, dev), metric), rt.prepare_dense(_t(xg, dev), metric)
    assert g.data.numel() * 4 == 192 * n * 4 and q.data.numel() == 64 * n   # whole blocks of 64 rows
    got = rt.dense_dist(q, g, metric)
    assert got.dtype == torch.float32 and got.shape == (9, 131)
    assert np.array_equal(dref.bits(got.cpu().numpy()), dref.bits(D.astype(np.float32)))
    # the layout of the header: block, dimension, row in block; the rows that fill the last block are zeros
    lay = g.data.cpu().numpy().reshape(3, n, 64)
    assert np.array_equal(lay.transpose(0, 2, 1).reshape(192, n)[:131], xg) and not lay.transpose(0, 2, 1).reshape(192, n)[131:].any()


# ---- exact inputs: top-k -----------------------------------------------------------------------------------------------------------
_SEG_CACHE = {}


def _seg_problem(metric):
    if metric not in _SEG_CACHE:
        rng = np.random.default_rng(200)
        xq, xg = _grid(rng, QN_SEG, 48), _grid(rng, G_SEG, 48)
        xg[rng.integers(0, G_SEG, 200)] = xg[rng.integers(0, G_SEG, 200)]      # duplicate rows on top of the grid's own ties
        D = dref.dist(xq, xg, metric)
        srt = np.sort(D, 1)
        assert int((srt[:, 1:] == srt[:, :-1]).sum()) > 5000            # the index tie-break does real work
        _SEG_CACHE[metric] = (xq, xg, D)
    return _SEG_CACHE[metric]


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_dense_topk_equals_lexsort_on_the_exact_grid(dev, metric, k):
    from concepthash_amd import retrieval as rt
    xq, xg, D = _seg_problem(metric)
    want = dref.topk(D, k)
    q, g = rt.prepare_dense(_t(xq, dev), metric), rt.prepare_dense(_t(xg, dev), metric)
    got = rt.dense_topk(q, g, metric, k, seg_rows=256)                   # three whole segments and a 3-row tail
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and _same_lists(got, want)
    assert _same_lists(rt.dense_topk(q, g, metric, k), want)            # the segmentation of the entry's own choice: one segment
    assert _same_lists(rt.dense_topk(q, g, metric, k, g_index_base=1000, seg_rows=256), dref.topk(D, k, base=1000))
    # the gallery cut in two, two calls, merged on the host by (ord(D), index) == one call
    cut = 300
    a = rt.dense_topk(q, rt.prepare_dense(_t(xg[:cut], dev), metric), metric, k, seg_rows=256)
    b = rt.dense_topk(q, rt.prepare_dense(_t(xg[cut:], dev), metric), metric, k, g_index_base=cut, seg_rows=256)
    merged = dref.merge_lists([a[0].cpu().numpy(), b[0].cpu().numpy()], [a[1].cpu().numpy(), b[1].cpu().numpy()], k)
    assert np.array_equal(merged[0], want[0]) and np.array_equal(dref.bits(merged[1]), dref.bits(want[1]))


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
def test_dense_topk_short_gallery_fills_with_minus_one_and_infinity(dev, metric):
    from concepthash_amd import retrieval as rt
    xq, xg, D = _seg_problem(metric)
    q = rt.prepare_dense(_t(xq, dev), metric)
    for rows in (5, 1, 0):
        want = dref.topk(D[:, :rows], 10)
        assert np.all(want[0][:, rows:] == -1) and np.all(np.isposinf(want[1][:, rows:]))
        assert _same_lists(rt.dense_topk(q, rt.prepare_dense(_t(xg[:rows], dev), metric), metric, 10), want), rows
    g = rt.prepare_dense(_t(xg, dev), metric)
    assert rt.dense_topk(rt.prepare_dense(_t(xq[:0], dev), metric), g, metric, 10)[0].shape == (0, 10)
    # the longest list over a gallery shorter than it: 100 hits, then 28 x (-1, +inf)
    rng = np.random.default_rng(128)
    yq, yg = _grid(rng, 3, 8), _grid(rng, 100, 8)
    want = dref.topk(dref.dist(yq, yg, metric), 128)
    assert np.all(want[0][:, :100] >= 0) and np.all(want[0][:, 100:] == -1) and np.all(np.isposinf(want[1][:, 100:]))
    assert _same_lists(rt.dense_topk(rt.prepare_dense(_t(yq, dev), metric), rt.prepare_dense(_t(yg, dev), metric), metric, 128), want)


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
def test_dense_topk_equal_rows_on_both_sides_of_a_segment_boundary_come_out_in_row_order(dev, metric):
    """rows 255, 256 and 257 are copies of one another and 256-row segments part them: their equal distances merge in row order"""
    from concepthash_amd import retrieval as rt
    xq, xg, _ = _seg_problem(metric)
    xg = xg.copy()
    xg[256] = xg[257] = xg[255] = xq[1]                                 # query 1 itself: the three are at the head of its list
    D = dref.dist(xq[:3], xg, metric)
    want = dref.topk(D, 128)
    assert np.array_equal(want[0][1][np.isin(want[0][1], (255, 256, 257))], (255, 256, 257))
    got = rt.dense_topk(rt.prepare_dense(_t(xq[:3], dev), metric), rt.prepare_dense(_t(xg, dev), metric), metric, 128, seg_rows=256)
    assert _same_lists(got, want)


# ---- exact inputs: the evaluation --------------------------------------------------------------------------------------------------
_EVAL_CACHE = {}


def _eval_problem(metric, multi):
    """grid codes, labels single or multi-hot with one query that has no relevant row, the fp64 (= exact) distances and the reference
    integers for every (R, remove_first) -- built once per (metric, label kind)"""
    key = (metric, multi)
    if key not in _EVAL_CACHE:
        rng = np.random.default_rng(300 + int(multi))
        xq, xg = _grid(rng, QN, 64), _grid(rng, G, 64)
        q_lab, g_lab = _labels(rng, multi)
        D = dref.dist(xq, xg, metric)
        srt = np.sort(D, 1)
        assert int((srt[:, 1:] == srt[:, :-1]).sum()) >= 100             # adjacent tied pairs
        rel = aref.relevance(q_lab, g_lab)
        want = {(R, rf): aref.evaluate(D, rel, [R] + list(KS), rf) for R in (-1, 50) for rf in (False, True)}
        assert want[(-1, False)][2][3] == 0
        _EVAL_CACHE[key] = (xq, xg, q_lab, g_lab, D, rel, want)
    return _EVAL_CACHE[key]


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("remove_first", [False, True])
def test_evaluate_dense_equals_the_brute_force_on_the_exact_grid(dev, metric, multi, remove_first):
    from concepthash_amd import retrieval as rt
    xq, xg, q_lab, g_lab, D, rel, want = _eval_problem(metric, multi)
    tq, tg, ql, gl = _t(xq, dev), _t(xg, dev), _t(q_lab, dev), _t(g_lab, dev)
    for R in (-1, 50):
        for seg_rows, list_cap in ((None, None), (256, 4), (65535, 8192)):    # list_cap 4: every list is searched in global memory
            out = rt.evaluate_dense(tq, tg, ql, gl, metric, R=R, ks=KS, remove_first=remove_first, seg_rows=seg_rows, list_cap=list_cap)
            _check_eval(out, want[(R, remove_first)], (R, seg_rows, list_cap))
    # more than 16 limits: the AP launch repeats
    Rs = [-1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16]
    many = rt.evaluate_dense(tq, tg, ql, gl, metric, R=Rs, ks=KS, remove_first=remove_first)
    S, nrel, total = aref.evaluate(D, rel, Rs + list(KS), remove_first)
    assert len(many["S"]) == len(Rs) and isinstance(many["mAP"], list)
    for i in range(len(Rs)):
        assert np.array_equal(many["S"][i].cpu().numpy().view(np.uint64), S[i]) and np.array_equal(many["nrel"][i].cpu().numpy(), nrel[i])
    assert np.array_equal(many["hits"].cpu().numpy(), nrel[len(Rs):].T) and np.array_equal(many["total"].cpu().numpy(), total)


@pytest.mark.parametrize("metric", ["dot", "euclidean"])
def test_two_gallery_shards_add_into_one_bins(dev, metric):
    from concepthash_amd import retrieval as rt
    xq, xg, q_lab, g_lab, D, rel, want = _eval_problem(metric, False)
    q, g = rt.prepare_dense(_t(xq, dev), metric), rt.prepare_dense(_t(xg, dev), metric)
    ql, gl, LW = rt.prepare_labels(_t(q_lab, dev), _t(g_lab, dev))
    offsets, keys, longest = rt.dense_rank_collect(q, g, ql, gl, LW)
    assert longest == int(rel.sum(1).max()) and keys.numel() == int(rel.sum())
    keys = rt.sort_slices_unsigned(offsets, keys)
    whole = rt.dense_rank_count(q, g, offsets, keys, longest)
    cut = 300
    bins = rt.dense_rank_count(q, rt.prepare_dense(_t(xg[:cut], dev), metric), offsets, keys, longest, seg_rows=256)
    bins = rt.dense_rank_count(q, rt.prepare_dense(_t(xg[cut:], dev), metric), offsets, keys, 4, g_index_base=cut, bins=bins)
    assert torch.equal(bins, whole) and int(whole.sum()) > 0
    limits, _ = rt.normalize_limits([-1] + list(KS))
    S, nrel, total = rt.rank_ap(offsets, bins, limits)
    ws, wn, wt = want[(-1, False)]
    order = [limits.index(0)] + [limits.index(k) for k in KS]
    assert np.array_equal(S.cpu().numpy().view(np.uint64)[order], ws) and np.array_equal(nrel.cpu().numpy()[order], wn)
    assert np.array_equal(total.cpu().numpy(), wt)


def test_sort_slices_unsigned_orders_keys_that_use_all_64_bits(dev):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(7)
    n = np.array([5, 0, 300, 1, 77])
    keys = rng.integers(0, 2 ** 64, int(n.sum()), dtype=np.uint64)
    keys[:5] = [2 ** 63, 2 ** 63 - 1, 0, 2 ** 64 - 1, 2 ** 63 + 1]
    offsets = np.r_[0, np.cumsum(n)]
    got = rt.sort_slices_unsigned(_t(offsets.astype(np.int64), dev), _t(keys.view(np.int64), dev)).cpu().numpy().view(np.uint64)
    want = np.concatenate([np.sort(keys[offsets[i]:offsets[i + 1]]) for i in range(n.size)])
    assert np.array_equal(got, want)
    d = torch.tensor([0.0, -0.0, 1.5, -1.5, 3e38, -3e38, 1.25e-30, -1.25e-30, float("inf")], device=dev)
    o = rt.dense_order(d)
    assert np.array_equal(o.cpu().numpy().astype(np.uint64), dref.order_key(d.cpu().numpy()))
    assert torch.equal(rt.dense_unorder(o).view(torch.int32), (d + 0.0).view(torch.int32))
    assert torch.equal(torch.argsort(o, stable=True), torch.argsort(d + 0.0, stable=True))


# ---- +-1 codes: the new path against the pinned Hamming one, through heavy ties ----------------------------------------------------
@pytest.mark.parametrize("metric,n", [("cosine", 16), ("cosine", 64), ("cosine", 256)] +
                         [(m, n) for m in ("dot", "euclidean") for n in (16, 48, 64, 120, 256)])
def test_sign_codes_rank_as_hamming_topk_and_evaluate(dev, metric, n):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(400 + n)
    C = 7
    centres = np.where(rng.random((C, n)) < 0.5, -1.0, 1.0)
    ql, gl = _labels(rng, False, C, QN_SEG, G_SEG)
    noisy = lambda lab: (centres[lab % C] * np.where(rng.random((lab.size, n)) < 0.1, -1.0, 1.0)).astype(np.float32)
    xq, xg = _t(noisy(ql), dev), _t(noisy(gl), dev)
    q, g = rt.prepare_dense(xq, metric), rt.prepare_dense(xg, metric)
    pq, pg = rt.pack_sign(xq), rt.pack_sign(xg)
    for k in (10, 128):
        idx, dist = rt.dense_topk(q, g, metric, k, seg_rows=256)
        hidx, hdist = rt.hamming_topk(pq, pg, k)
        assert torch.equal(idx, hidx)
        h = hdist.to(torch.float32)
        want = {"dot": 2 * h - n, "euclidean": 4 * h, "cosine": 2 * h / n}[metric]       # exact in fp32: 1 / sqrt(n) is a power of two
        assert torch.equal(dist, want)
    tql, tgl = _t(ql, dev), _t(gl, dev)
    for rf in (False, True):
        out = rt.evaluate_dense(xq, xg, tql, tgl, metric, R=-1, ks=KS, remove_first=rf, seg_rows=256)
        ham = rt.evaluate(pq, pg, tql, tgl, R=-1, ks=KS, remove_first=rf)
        for key in ("S", "nrel", "total", "hits"):
            assert torch.equal(out[key], ham[key]), (key, rf)
        assert out["mAP"] == ham["mAP"] and out["precisions"] == ham["precisions"] and out["recalls"] == ham["recalls"]


# ---- gaussian codes: one distance in every pass --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", dref.METRICS)
@pytest.mark.parametrize("n", [48, 64, 256])
def test_every_pass_computes_the_same_bits(dev, metric, n):
    """The distance matrix, the top-k scan (16 queries per tile, any segmentation), the collect pass and -- through the ranks it counts --
    the count pass: a relevant row is ranked against its own collected key, so one ulp between two passes moves a rank by one."""
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(500 + n)
    xq, xg = rng.standard_normal((QN, n)).astype(np.float32), rng.standard_normal((G, n)).astype(np.float32)
    q_lab, g_lab = _labels(rng, False)
    q, g = rt.prepare_dense(_t(xq, dev), metric), rt.prepare_dense(_t(xg, dev), metric)
    M = rt.dense_dist(q, g, metric).cpu().numpy()
    assert np.all(np.abs(M - dref.dist(xq, xg, metric)) <= dref.bound(xq, xg, metric))
    for seg_rows in (256, None):
        idx, dist = rt.dense_topk(q, g, metric, 10, seg_rows=seg_rows)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        assert np.array_equal(dref.bits(dist), dref.bits(np.take_along_axis(M, idx, 1)))
        assert np.array_equal(idx, dref.topk(M.astype(np.float64), 10)[0])            # ... and ranks by them
    ql, gl, LW = rt.prepare_labels(_t(q_lab, dev), _t(g_lab, dev))
    offsets, keys, _ = rt.dense_rank_collect(q, g, ql, gl, LW)
    off, keys = offsets.cpu().numpy(), keys.cpu().numpy().view(np.uint64)
    rel = aref.relevance(q_lab, g_lab)
    for i in range(QN):
        sl = keys[off[i]:off[i + 1]]
        rows = (sl & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert sorted(rows.tolist()) == np.flatnonzero(rel[i]).tolist()
        assert np.array_equal(sl >> np.uint64(32), dref.order_key(M[i, rows])), i
        back = rt.dense_unorder(torch.from_numpy((sl >> np.uint64(32)).astype(np.int64))).numpy()
        assert np.array_equal(dref.bits(back), dref.bits(M[i, rows]))
    for rf in (False, True):
        out = rt.evaluate_dense(_t(xq, dev), _t(xg, dev), _t(q_lab, dev), _t(g_lab, dev), metric, R=-1, ks=KS, remove_first=rf, seg_rows=256)
        _check_eval(out, aref.evaluate(M.astype(np.float64), rel, [-1] + list(KS), rf), rf)


# ---- clustered gaussian codes against fp64 within the derived bounds ---------------------------------------------------------------
_REAL_CACHE = {}


def _real_problem(n):
    if n not in _REAL_CACHE:
        rng = np.random.default_rng(0)
        C = 7
        centres = np.where(rng.random((C, n)) < 0.5, -1.0, 1.0)
        gl, ql = rng.integers(0, C, G), rng.integers(0, C, QN)
        _REAL_CACHE[n] = (aref.clustered_codes(rng, QN, n, ql, centres), aref.clustered_codes(rng, G, n, gl, centres), ql, gl)
    return _REAL_CACHE[n]


@pytest.mark.parametrize("metric", dref.METRICS)
@pytest.mark.parametrize("n", [16, 64])
def test_topk_on_real_codes_lies_within_the_bounds_of_fp64(dev, metric, n):
    from concepthash_amd import retrieval as rt
    xq, xg, ql, gl = _real_problem(n)
    k = 10
    D, E = dref.dist(xq, xg, metric), dref.bound(xq, xg, metric)
    q, g = rt.prepare_dense(_t(xq, dev), metric), rt.prepare_dense(_t(xg, dev), metric)
    idx, dist = rt.dense_topk(q, g, metric, k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.all(np.abs(dist - np.take_along_axis(D, idx, 1)) <= np.take_along_axis(E, idx, 1))
    key = dref.order_key(dist) << np.uint64(32) | idx.astype(np.uint64)
    assert np.all(key[:, 1:] > key[:, :-1])                             # ascending (ord(D), index)
    # E of a query: its largest over the rows.  A row r with D_r < kth - 2 E has an fp32 distance below kth - E, and the fp32 distance
    # of every row s with D_s >= kth is at least kth - E: fewer than k rows can come before r.  The mirror image bounds what is returned.
    kth, Emax = np.sort(D, 1)[:, k - 1], E.max(1)
    for i in range(QN):
        inside = np.zeros(G, bool)
        inside[idx[i]] = True
        assert np.all(inside[D[i] < kth[i] - 2 * Emax[i]]), i          # every row clearly below the k-th smallest is in the list
        assert np.all(D[i, idx[i]] <= kth[i] + 2 * Emax[i]), i         # and no returned row lies clearly above it


@pytest.mark.parametrize("metric", dref.METRICS)
@pytest.mark.parametrize("n", [16, 64])
def test_ap_on_real_codes_lies_inside_the_bracket_of_fp64(dev, metric, n):
    from concepthash_amd import retrieval as rt
    xq, xg, ql, gl = _real_problem(n)
    lo, hi = dref.ap_bracket(dref.dist(xq, xg, metric), dref.bound(xq, xg, metric), aref.relevance(ql, gl))
    print(f"{metric} n={n}: bracket width max {float((hi - lo).max()):.3e} mean {float((hi - lo).mean()):.3e}")
    assert np.all(hi - lo <= 1e-3)                                      # a condition: the bracket must not swallow a wrong ranking
    out = rt.evaluate_dense(_t(xq, dev), _t(xg, dev), _t(ql, dev), _t(gl, dev), metric, R=-1, ks=KS)
    ap = out["ap"].cpu().numpy()
    # 1e-9: the 2^-32 fixed-point quotient times at most 700 terms, normalised
    assert np.all(ap >= lo - 1e-9) and np.all(ap <= hi + 1e-9), (float((lo - ap).max()), float((ap - hi).max()))
    assert abs(out["mAP"] - float(ap.mean())) < 1e-12


# ---- surfaces ----------------------------------------------------------------------------------------------------------------------
def test_calculate_map_and_pr_curve_under_a_dense_rank_equal_evaluate_dense(dev):
    from concepthash_amd import retrieval as rt
    from utils import hashing
    xq, xg, ql, gl = _real_problem(64)
    ql = ql.copy()
    ql[3] = 7                                                           # a class no database row has
    qoh, goh = torch.eye(8)[ql], torch.eye(8)[gl]                       # one-hot CPU tensors, as the evaluator passes them
    qc, gc = torch.from_numpy(xq), torch.from_numpy(xg)
    for R, rf in ((-1, False), (50, True)):
        want = rt.evaluate_dense(_t(xq, dev), _t(xg, dev), _t(ql, dev), _t(gl, dev), "cosine", R=R, ks=KS, remove_first=rf)
        mAP, recalls, precisions = hashing.calculate_mAP(gc, goh, qc, qoh, R, PRs=list(KS), rank="cosine", remove_first_retrieved=rf)
        assert mAP == want["mAP"] and recalls == want["recalls"] and precisions == want["precisions"]
    many = hashing.calculate_mAP(gc, goh, qc, qoh, [50, -1], PRs=list(KS), rank="cosine", remove_first_retrieved=True)
    assert many[0][0] == want["mAP"] and isinstance(many[0], list)
    skipped, _, _ = hashing.calculate_mAP(gc, goh, qc, qoh, -1, rank="cosine", skip_queries_without_relevant=True)
    plain, _, _ = hashing.calculate_mAP(gc, goh, qc, qoh, -1, rank="cosine")
    assert abs(skipped - plain * QN / (QN - 1)) < 1e-12
    assert hashing.last_tie_bracket is None and hashing.last_hash_lookup is None
    depths = [1, 10, 100, 700]
    recalls, precisions, Rs = hashing.calculate_pr_curve(gc, goh, qc, qoh, Rs=depths, rank="euclidean")
    ev = rt.evaluate_dense(_t(xq, dev), _t(xg, dev), _t(ql, dev), _t(gl, dev), "euclidean", R=depths, ks=[])
    total = ev["total"].double()
    assert Rs == depths
    for i, r in enumerate(depths):
        assert precisions[i] == float((ev["nrel"][i].double() / r).mean())
        assert recalls[i] == float(torch.where(total > 0, ev["nrel"][i].double() / total.clamp_min(1), torch.zeros_like(total)).mean())
    assert recalls[-1] == pytest.approx((QN - 1) / QN)                  # every relevant row is inside the whole database


def test_gallery_index_search_under_a_dense_rank_returns_the_dense_topk_rows(dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    xq, xg, ql, gl = _real_problem(64)
    gt = _t(xg, dev)
    mean = gt.mean(0)
    index = GalleryIndex(rt.pack_sign(gt - mean), 64, 4, labels=_t(gl, dev), mean=mean, real=gt - mean)
    for rank in dref.METRICS:
        res = index.search(torch.from_numpy(xq), 10, rank=rank)         # the index's mean is applied to the queries
        q, g = rt.prepare_dense(_t(xq, dev) - mean, rank), rt.prepare_dense(gt - mean, rank)
        idx, dist = rt.dense_topk(q, g, rank, 10)
        assert torch.equal(res["idx"], idx) and torch.equal(res["dist"], dist) and res["dist"].dtype == torch.float32 and res["rank"] == rank
        assert torch.equal(res["labels"], _t(gl, dev)[idx]) and res["bits"].tolist() == [64] * QN
        ham = (np.where(xq - mean.cpu().numpy() > 0, 1, 0)[:, None, :] != np.where(xg - mean.cpu().numpy() > 0, 1, 0)[None, :, :])
        cd = res["concept_dist"].cpu().numpy()                          # the hits' sign codes, concept by concept
        for i in range(QN):
            assert np.array_equal(cd[i].sum(1), ham[i, idx[i].cpu().numpy()].sum(1))
    text = index.search(torch.from_numpy(xq), 10, rank="euclidean", mean_shift=False)          # text queries are never shifted
    idx, dist = rt.dense_topk(rt.prepare_dense(_t(xq, dev), "euclidean"), rt.prepare_dense(gt - mean, "euclidean"), "euclidean", 10)
    assert torch.equal(text["idx"], idx) and torch.equal(text["dist"], dist)
    short = GalleryIndex(rt.pack_sign(gt[:4]), 64, 4, real=gt[:4]).search(torch.from_numpy(xq), 6, rank="dot")
    assert bool((short["idx"][:, 4:] == -1).all()) and bool(torch.isposinf(short["dist"][:, 4:]).all()) and short["labels"] is None


COMMON = ["dataset=synthetic_cub200", "dataset.limit=96", "batch_size=32"]


def _main_v2(args, cwd):
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py")] + args, check=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=cwd,
                   timeout=600)


def test_the_search_and_the_validation_commands_under_a_dense_rank(tmp_path, dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    logdir = str(tmp_path / "run")
    common = COMMON + ["data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path))
    ev0, ev, s0, s1 = str(tmp_path / "ev0"), str(tmp_path / "ev"), str(tmp_path / "s0"), str(tmp_path / "s1")
    _main_v2(["--config-name", "val.yaml", "logdir=" + logdir, "save_code=True", "eval_logdir=" + ev0] + common, str(tmp_path))
    outs = torch.load(os.path.join(ev0, "outputs.pth"))
    te, db = outs["test"], outs["db"]
    # exp=search: a Hamming search leaves an index without the plane; rank=cosine rebuilds it with the plane by itself
    _main_v2(["--config-name", "search.yaml", "logdir=" + logdir, "search_logdir=" + s0, "k=5"] + common, str(tmp_path))
    assert GalleryIndex.load(os.path.join(logdir, "index_best.pth")).real is None
    _main_v2(["--config-name", "search.yaml", "logdir=" + logdir, "search_logdir=" + s1, "rank=cosine", "k=5"] + common, str(tmp_path))
    res = json.load(open(os.path.join(s1, "results.json")))
    assert res["rank"] == "cosine" and res["k"] == 5 and res["index_rows"] == 96 and res["index_status"].startswith("built: stale index")
    saved = GalleryIndex.load(os.path.join(logdir, "index_best.pth"))
    gt = db["codes"].to(dev, torch.float32)
    assert saved.real is not None and torch.equal(saved.real, gt.cpu()) and torch.equal(saved.codes, rt.pack_sign(gt).cpu())
    direct = GalleryIndex(rt.pack_sign(gt), 64, res["ncontext"], real=gt).search(te["codes"], 5, rank="cosine")
    idx, dist, cd = direct["idx"].tolist(), direct["dist"].tolist(), direct["concept_dist"].tolist()
    assert len(res["queries"]) == 96
    for i, e in enumerate(res["queries"]):
        assert [h["index"] for h in e["hits"]] == idx[i] and [h["distance"] for h in e["hits"]] == dist[i], i
        assert [h["concept_distances"] for h in e["hits"]] == cd[i] and e["distance_max"] is None and e["unmasked_bits"] == 64
    # val.yaml dense_eval=true dense_metric=cosine
    _main_v2(["--config-name", "val.yaml", "logdir=" + logdir, "dense_eval=true", "dense_metric=cosine", "eval_logdir=" + ev] + common,
             str(tmp_path))
    hist = json.load(open(os.path.join(ev, "history.json")))
    base = json.load(open(os.path.join(ev0, "history.json")))
    for key in ("mAP_dense", "recalls_dense", "precisions_dense", "dense_metric", "quantisation_gap"):
        assert key in hist and key not in base, key
    for key, v in base.items():                                         # every existing key's value is what it was
        assert key in hist, key
        if key.startswith(("test_", "db_")):                            # the two encode passes' loss / accuracy meters: run to run
            assert hist[key] == pytest.approx(v, rel=1e-6), key
        elif key != "timing_s":
            assert hist[key] == v, key
    assert hist["dense_metric"] == "cosine" and hist["quantisation_gap"] == hist["mAP_dense"] - hist["mAP"]
    want = rt.evaluate_dense(te["codes"].to(dev), gt, te["labels"].to(dev), db["labels"].to(dev), "cosine", R=-1, ks=(1, 5, 10))   # val.yaml: R, PRs
    assert hist["mAP_dense"] == want["mAP"] and hist["recalls_dense"] == want["recalls"] and hist["precisions_dense"] == want["precisions"]
