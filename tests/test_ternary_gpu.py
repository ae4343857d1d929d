"""GPU: ternary codes (csrc/hamming_ternary.hip) -- ch_pack_ternary, ch_ternary_dist, ch_ternary_topk and the
rank-counting evaluation under K against the numpy reference of tests/ternary_ref.py (K from the definition on unpacked codes), at the
smallest shapes that reach every path of the kernels; `calculate_mAP(rank="ternary")`, `GalleryIndex.search(rank="ternary")` and the two
`main_v2.py` commands on a synthetic run directory.  All arithmetic is integer: every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import asymmetric_eval_ref as aref
import ternary_ref as tref
from conftest import ROOT

pytestmark = pytest.mark.gpu

G_TIES = 771              # 256-row segments: three whole ones and a 3-row tail
QN_TIES = 70              # a partial wave of one query tile
MARGIN = 0.5
NBITS = {1: 56, 2: 120, 3: 184, 4: 256}     # W -> nbit: three code lengths that end inside a word, and the longest


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _same(got, want):
    return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


# ---- the packer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbit", [48, 64, 120, 256])
@pytest.mark.parametrize("margin", [0.0, 0.37])
def test_pack_ternary_equals_the_reference_and_its_two_identities(dev, nbit, margin):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(100 + nbit)
    x = rng.standard_normal((70, nbit)).astype(np.float32)
    m = np.float32(margin)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, m, -m, np.nextafter(m, np.float32(np.inf)), -np.nextafter(m, np.float32(np.inf))],
                       dtype=np.float32)
    x[0, :special.size] = special                     # +-margin exactly are ternary 0: the comparison is strict
    x[1] = 0.0
    x[2] = np.nan
    x[3, ::3] = m
    x[4, 1::2] = -m
    xt = torch.from_numpy(x).to(dev)
    got = rt.pack_ternary(xt, margin)
    assert got.shape == (70, 2, (nbit + 63) // 64) and got.dtype == torch.int64 and got.is_contiguous()
    t = tref.ternarise(x, margin)
    assert t[0, :special.size].tolist() == [0, 0, 0, 1, -1, 0, 0, 1, -1]
    assert np.array_equal(_u64(got), tref.planes(t))
    mask = rt.confidence_mask(xt, margin)
    assert torch.equal(got[:, 1], mask) and torch.equal(got[:, 0], rt.pack_sign(xt, 0.0) & mask)
    if nbit % 64:                                       # bits past nbit are zero in both planes
        assert not bool((got[:, :, -1] >> (nbit % 64)).ne(0).any())


# ---- the distance matrix -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbit", [48, 64, 120, 184, 256])
def test_ternary_dist_equals_the_definition(dev, nbit):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(200 + nbit)
    xq, xg = rng.standard_normal((9, nbit)).astype(np.float32), rng.standard_normal((131, nbit)).astype(np.float32)
    xg[5] = 0.0                                                         # an all-zero row: K = nbit against everything
    xq[2] = np.where(rng.random(nbit) < 0.5, -2.0, 2.0)                 # no zeros ...
    xg[7] = -xq[2]                                                      # ... and its exact opposite: K = 2 nbit
    tq, tg = tref.ternarise(xq, MARGIN), tref.ternarise(xg, MARGIN)
    K = tref.dist(tq, tg)
    assert np.all(K[:, 5] == nbit) and K[2, 7] == 2 * nbit and (nbit != 256 or K[2, 7] == 512)
    q3, g3 = rt.pack_ternary(torch.from_numpy(xq).to(dev), MARGIN), rt.pack_ternary(torch.from_numpy(xg).to(dev), MARGIN)
    got = rt.ternary_dist(q3, g3, nbit)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), K)


# ---- top-k -------------------------------------------------------------------------------------------------------------------------
def _tie_codes(nbit, seed):
    """Real codes whose ternary distances tie heavily: 5 class centres (+-1, with a fifth of their entries unsure); a gallery row is its
    class centre with ONE sure entry flipped, a query its class centre with a third of the entries unsure.  Against a query of its class a
    row is at the query's base distance if the flipped entry is one the query is unsure of, 2 above it otherwise: two levels of some
    50 and 100 rows, so every list of up to 128 ends inside a level.  Query 0 has no unsure entry, gallery row 99 is its exact opposite."""
    rng = np.random.default_rng(seed)
    C = 5
    centres = np.where(rng.random((C, nbit)) < 0.5, -1.0, 1.0)
    unsure = rng.random((C, nbit)) < 0.2
    gl, ql = np.arange(G_TIES) % C, np.arange(QN_TIES) % C
    g = centres[gl] * np.where(unsure[gl], 0.1, 1.0)
    for r in range(G_TIES):
        sure = np.flatnonzero(~unsure[gl[r]])
        g[r, sure[rng.integers(0, sure.size)]] *= -1.0
    q = centres[ql] * np.where(rng.random((QN_TIES, nbit)) < 1 / 3, 0.1, 1.0)
    q[0] = centres[0]
    g[99] = -q[0]
    return q.astype(np.float32), g.astype(np.float32)


_TIE_CACHE = {}


def _tie_problem(W):
    """(xq, xg, K from the definition) of the tie problem at W words, built once"""
    if W not in _TIE_CACHE:
        xq, xg = _tie_codes(NBITS[W], 300 + W)
        tq, tg = tref.ternarise(xq, MARGIN), tref.ternarise(xg, MARGIN)
        for t in (tq, tg):                                              # the zero share on both sides
            assert 0.10 <= float((t == 0).mean()) <= 0.60
        _TIE_CACHE[W] = (xq, xg, tref.dist(tq, tg))
    return _TIE_CACHE[W]


@pytest.mark.parametrize("W", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_ternary_topk_equals_the_reference_under_heavy_ties(dev, W, k):
    from concepthash_amd import retrieval as rt
    nbit = NBITS[W]
    xq, xg, K = _tie_problem(W)
    want = tref.topk(K, k)
    # the index order does real work: at least a quarter of every query's list is tied with a row outside the list
    for i in range(QN_TIES):
        outside = np.delete(K[i], want[0][i])
        tied = np.isin(want[1][i], outside).sum()
        assert 4 * tied >= k, (i, tied)
    assert K[0].min() < K[0].max()
    q3, g3 = rt.pack_ternary(torch.from_numpy(xq).to(dev), MARGIN), rt.pack_ternary(torch.from_numpy(xg).to(dev), MARGIN)
    got = rt.ternary_topk(q3, g3, nbit, k)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and _same(got, want)
    # a non-zero g_index_base; the gallery cut in two, two calls, ch_topk_merge == one call
    assert _same(rt.ternary_topk(q3, g3, nbit, k, g_index_base=1000), tref.topk(K, k, base=1000))
    cut = 300
    a = rt.ternary_topk(q3, g3[:cut], nbit, k)
    b = rt.ternary_topk(q3, g3[cut:], nbit, k, g_index_base=cut)
    assert _same(rt.topk_merge(torch.stack([a[0], b[0]]), torch.stack([a[1], b[1]])), want)


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_ternary_topk_short_gallery_fills_with_minus_one_and_ranks_the_opposite_row_last(dev, W):
    from concepthash_amd import retrieval as rt
    nbit = NBITS[W]
    xq, xg, K = _tie_problem(W)
    q3, g3 = rt.pack_ternary(torch.from_numpy(xq).to(dev), MARGIN), rt.pack_ternary(torch.from_numpy(xg[:100]).to(dev), MARGIN)
    want = tref.topk(K[:, :100], 128)
    assert np.all(want[0][:, 100:] == -1) and want[0][0, 99] == 99 and want[1][0, 99] == 2 * nbit and (W != 4 or want[1][0, 99] == 512)
    got = rt.ternary_topk(q3, g3, nbit, 128)
    assert _same(got, want)
    for G in (0, 1, 3, 5):                              # an empty gallery; fewer rows than one block of the scan
        assert _same(rt.ternary_topk(q3, g3[:G], nbit, 10), tref.topk(K[:, :G], 10))
    assert rt.ternary_topk(q3[:0], g3, nbit, 10)[0].shape == (0, 10)


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_sure_codes_rank_as_hamming_topk_with_twice_its_distance(dev, W):
    from concepthash_amd import retrieval as rt
    nbit = NBITS[W]
    rng = np.random.default_rng(400 + W)
    centres = np.where(rng.random((5, nbit)) < 0.5, -1.0, 1.0)
    noisy = lambda rows: (centres[np.arange(rows) % 5] * np.where(rng.random((rows, nbit)) < 0.08, -1.0, 1.0) *
                          rng.uniform(0.6, 2.0, (rows, nbit))).astype(np.float32)              # every |x| > margin
    xq, xg = torch.from_numpy(noisy(QN_TIES)).to(dev), torch.from_numpy(noisy(G_TIES)).to(dev)
    q3, g3 = rt.pack_ternary(xq, MARGIN), rt.pack_ternary(xg, MARGIN)
    for k in (10, 128):
        idx, dist = rt.ternary_topk(q3, g3, nbit, k)
        hidx, hdist = rt.hamming_topk(rt.pack_sign(xq), rt.pack_sign(xg), k)
        assert torch.equal(idx, hidx) and torch.equal(dist, 2 * hdist)


# ---- the evaluation ----------------------------------------------------------------------------------------------------------------
KS = (1, 5, 10)
_EVAL_CACHE = {}


def _eval_problem(multi):
    """codes of 7 classes (centres +-1 plus noise), labels single or multi-hot with one query that has no relevant row, K from the
    definition and the reference integers for every (R, remove_first) -- built once per label kind"""
    if multi not in _EVAL_CACHE:
        rng = np.random.default_rng(500 + int(multi))
        nbit, C = 120, 7
        centres = np.where(rng.random((C, nbit)) < 0.5, -1.0, 1.0)
        gl, ql = rng.integers(0, C, G_TIES), rng.integers(0, C, QN_TIES)
        xg, xq = aref.clustered_codes(rng, G_TIES, nbit, gl, centres), aref.clustered_codes(rng, QN_TIES, nbit, ql, centres)
        xg[rng.integers(0, G_TIES, 200)] = xg[rng.integers(0, G_TIES, 200)]      # duplicate rows: equal K is common
        if multi:
            q_lab, g_lab = np.eye(C, dtype=np.int64)[ql], np.eye(C, dtype=np.int64)[gl]
            g_lab[rng.random((G_TIES, C)) < 0.1] = 1
            q_lab[rng.random((QN_TIES, C)) < 0.1] = 1
            q_lab[3] = 0                                                    # no class at all: no relevant row
        else:
            q_lab, g_lab = ql.copy(), gl.copy()
            q_lab[3] = C                                                    # a class the gallery does not hold
        tq, tg = tref.ternarise(xq, MARGIN), tref.ternarise(xg, MARGIN)
        assert 0.10 <= float((tq == 0).mean()) <= 0.60 and 0.10 <= float((tg == 0).mean()) <= 0.60
        K = tref.dist(tq, tg)
        want = {(R, rf): tref.evaluate(K, q_lab, g_lab, [R] + list(KS), rf) for R in (-1, 50) for rf in (False, True)}
        assert want[(-1, False)][2][3] == 0
        _EVAL_CACHE[multi] = (xq, xg, q_lab, g_lab, nbit, want)
    return _EVAL_CACHE[multi]


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("R", [-1, 50])
@pytest.mark.parametrize("remove_first", [False, True])
def test_evaluate_ternary_equals_the_reference(dev, multi, R, remove_first):
    from concepthash_amd import retrieval as rt
    xq, xg, q_lab, g_lab, nbit, want = _eval_problem(multi)
    S, nrel, total = want[(R, remove_first)]
    mAPs, prec, rec = tref.summarize(S, nrel, total, 1, KS)
    q3, g3 = rt.pack_ternary(torch.from_numpy(xq).to(dev), MARGIN), rt.pack_ternary(torch.from_numpy(xg).to(dev), MARGIN)
    ql, gl = torch.from_numpy(q_lab).to(dev), torch.from_numpy(g_lab).to(dev)
    for seg_rows in (256, 65535):
        for list_cap in (1, 8192):                      # every list in global memory / every list in LDS
            out = rt.evaluate_ternary(q3, g3, nbit, ql, gl, R=R, ks=KS, remove_first=remove_first, seg_rows=seg_rows, list_cap=list_cap)
            where = (seg_rows, list_cap)
            assert np.array_equal(out["S"].cpu().numpy().view(np.uint64), S[0]), where
            assert np.array_equal(out["nrel"].cpu().numpy(), nrel[0]) and np.array_equal(out["total"].cpu().numpy(), total), where
            assert np.array_equal(out["hits"].cpu().numpy(), nrel[1:].T), where
            assert abs(out["mAP"] - mAPs[0]) < 1e-12 and np.allclose(out["precisions"], prec, rtol=0, atol=1e-12), where
            assert np.allclose(out["recalls"], rec, rtol=0, atol=1e-12), where
    both = rt.evaluate_ternary(q3, g3, nbit, ql, gl, R=[50, -1], ks=KS, remove_first=remove_first)       # the defaults; a list R
    assert np.array_equal(both["S"][0 if R == 50 else 1].cpu().numpy().view(np.uint64), S[0])


def test_calculate_map_under_the_ternary_rank_equals_the_reference():
    from utils import hashing
    xq, xg, q_lab, g_lab, nbit, want = _eval_problem(False)
    C = 8                                               # query 3 carries class 7, which no database row has
    qoh, goh = torch.eye(C)[q_lab], torch.eye(C)[g_lab]                  # one-hot CPU tensors, as the evaluator passes them
    qc, gc = torch.from_numpy(xq), torch.from_numpy(xg)
    for R, rf in ((-1, False), (50, True)):
        mAPs, prec, rec = tref.summarize(*want[(R, rf)], 1, KS)
        mAP, recalls, precisions = hashing.calculate_mAP(gc, goh, qc, qoh, R, PRs=list(KS), rank="ternary", margin=MARGIN,
                                                         remove_first_retrieved=rf)
        assert abs(mAP - mAPs[0]) < 1e-12 and np.allclose(recalls, rec, rtol=0, atol=1e-12)
        assert np.allclose(precisions, prec, rtol=0, atol=1e-12)
    skipped, _, _ = hashing.calculate_mAP(gc, goh, qc, qoh, -1, rank="ternary", margin=MARGIN, skip_queries_without_relevant=True)
    assert abs(skipped - tref.summarize(*want[(-1, False)], 1, KS)[0][0] * QN_TIES / (QN_TIES - 1)) < 1e-12
    assert hashing.last_tie_bracket is None and hashing.last_hash_lookup is None


# ---- the index and the two commands ------------------------------------------------------------------------------------------------
def test_gallery_index_search_ranks_by_k_with_concepts_and_radius(dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    nbit, Q = 120, 3
    xq, xg, _ = _tie_problem(2)
    xq, xg = xq[:9], xg[:200]
    gt = torch.from_numpy(xg).to(dev)
    index = GalleryIndex(rt.pack_sign(gt), nbit, Q, labels=torch.arange(200, device=dev) % 5, mask=rt.confidence_mask(gt, 0.3), margin=0.3)
    tq, tg = tref.ternarise(xq, MARGIN), tref.ternarise(xg, 0.3)
    res = index.search(torch.from_numpy(xq), 10, margin=MARGIN, rank="ternary")
    want = tref.topk(tref.dist(tq, tg), 10)
    assert _same((res["idx"], res["dist"]), want) and res["rank"] == "ternary" and res["index_margin"] == 0.3
    assert np.array_equal(res["dist_bits"].cpu().numpy(), want[1] / 2) and res["bits"].tolist() == (tq != 0).sum(1).tolist()
    assert res["dist_max"].tolist() == ((tq != 0).sum(1) + nbit).tolist()
    ham = (np.where(xq > 0, 1, 0)[:, None, :] != np.where(xg > 0, 1, 0)[None, :, :])                  # sub_dist stays plain Hamming
    cd = res["concept_dist"].cpu().numpy()
    for i in range(9):
        assert np.array_equal(cd[i].sum(1), ham[i, want[0][i]].sum(1))
    # concepts: the query is unsure of everything outside them and only their bits are in play
    sl = np.r_[0:40, 80:120]
    sub = index.search(torch.from_numpy(xq), 10, concepts=[0, 2], margin=MARGIN, rank="ternary")
    want_sub = tref.topk(tref.dist(tq[:, sl], tg[:, sl]), 10)
    assert _same((sub["idx"], sub["dist"]), want_sub) and sub["bits"].tolist() == (tq[:, sl] != 0).sum(1).tolist()
    # radius r keeps K <= 2 r
    r = int(np.median(want[1])) // 2
    cut = index.search(torch.from_numpy(xq), 10, margin=MARGIN, rank="ternary", radius=r)
    far = want[1] > 2 * r
    assert far.any() and not far.all()
    assert _same((cut["idx"], cut["dist"]), (np.where(far, -1, want[0]), np.where(far, -1, want[1])))


COMMON = ["dataset=synthetic_cub200", "dataset.limit=96", "batch_size=32"]


def _main_v2(args, cwd):
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py")] + args, check=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=cwd,
                   timeout=600)


def test_the_search_and_the_validation_commands_under_the_ternary_rank(tmp_path, dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    logdir = str(tmp_path / "run")
    common = COMMON + ["data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path))
    ev0, ev, s1 = str(tmp_path / "ev0"), str(tmp_path / "ev"), str(tmp_path / "s1")
    _main_v2(["--config-name", "val.yaml", "logdir=" + logdir, "save_code=True", "eval_logdir=" + ev0] + common, str(tmp_path))
    outs = torch.load(os.path.join(ev0, "outputs.pth"))
    te, db = outs["test"], outs["db"]
    m = float(db["codes"].abs().median())               # the scale of the codes belongs to the run
    assert m > 0
    # exp=search rank=ternary
    _main_v2(["--config-name", "search.yaml", "logdir=" + logdir, "search_logdir=" + s1, "rank=ternary", f"index_margin={m!r}",
              f"query_margin={m!r}", "k=10"] + common, str(tmp_path))
    res = json.load(open(os.path.join(s1, "results.json")))
    assert res["rank"] == "ternary" and res["index_margin"] == m and res["query_margin"] == m and res["k"] == 10 and res["index_rows"] == 96
    gt = db["codes"].to(dev)
    index = GalleryIndex(rt.pack_sign(gt), 64, res["ncontext"], mask=rt.confidence_mask(gt, m), margin=m)
    direct = index.search(te["codes"], 10, margin=m, rank="ternary")
    idx, dist, cd = direct["idx"].tolist(), direct["dist"].tolist(), direct["concept_dist"].tolist()
    assert len(res["queries"]) == 96
    for i, e in enumerate(res["queries"]):
        assert [h["index"] for h in e["hits"]] == idx[i] and [h["distance"] for h in e["hits"]] == dist[i], i
        assert [h["distance_bits"] for h in e["hits"]] == [d / 2 for d in dist[i]] and [h["concept_distances"] for h in e["hits"]] == cd[i]
        assert e["unmasked_bits"] == direct["bits"][i].item() and e["distance_max"] == direct["dist_max"][i].item()
    saved = GalleryIndex.load(os.path.join(logdir, "index_best.pth"))
    assert saved.margin == m and torch.equal(saved.mask, index.mask.cpu()) and torch.equal(saved.codes, index.codes.cpu())
    # val.yaml ternary_eval=true
    _main_v2(["--config-name", "val.yaml", "logdir=" + logdir, "ternary_eval=true", f"ternary_margin={m!r}", "eval_logdir=" + ev] + common,
             str(tmp_path))
    hist = json.load(open(os.path.join(ev, "history.json")))
    base = json.load(open(os.path.join(ev0, "history.json")))
    for key in ("mAP_ternary", "recalls_ternary", "precisions_ternary", "ternary_margin", "ternary_zero_share"):
        assert key in hist and key not in base, key
    assert hist["mAP"] == base["mAP"] and hist["ternary_margin"] == m
    q3, g3 = rt.pack_ternary(te["codes"].to(dev), m), rt.pack_ternary(gt, m)
    want = rt.evaluate_ternary(q3, g3, 64, te["labels"].to(dev), db["labels"].to(dev), R=-1, ks=(1, 5, 10))   # val.yaml: R, PRs
    assert hist["mAP_ternary"] == want["mAP"] and hist["recalls_ternary"] == want["recalls"] and hist["precisions_ternary"] == want["precisions"]
    share = lambda c: 1.0 - float((c.abs() > m).double().mean())
    assert hist["ternary_zero_share"] == [share(db["codes"]), share(te["codes"])] and 0.4 < hist["ternary_zero_share"][0] < 0.6

