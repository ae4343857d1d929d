"""GPU: the weighted (asymmetric) ranking -- ch_weight_planes and ch_hamming_topk_weighted against the numpy reference
(tests/weighted_topk_ref.py), at the smallest shapes that reach every path of the kernels; GalleryIndex.search(rank="asymmetric") and
`main_v2.py --config-name search.yaml rank=asymmetric` on a synthetic run directory.  All arithmetic is integer: every comparison is
exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import weighted_topk_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

G_TIES = 771              # 256-row segments: three whole ones and a 3-row tail
QN_TIES = 70


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _same(got, want):
    return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


def _mask_words(rng, rows, nbit):
    """random masks [rows, W] uint64; bits past nbit SET in half of the rows (they must not count)"""
    W = (nbit + 63) // 64
    m = rng.integers(0, 1 << 63, (rows, W), dtype=np.uint64) ^ (rng.integers(0, 2, (rows, W), dtype=np.uint64) << np.uint64(63))
    if nbit % 64:
        m[::2, -1] |= ~np.uint64((1 << (nbit % 64)) - 1)
    return m


# ---- planes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbit", [48, 64, 120, 256])
@pytest.mark.parametrize("bits", [4, 8])
def test_weight_planes_equal_the_reference(dev, nbit, bits):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(1000 + nbit + bits)
    Qn, L, W = 70, (1 << bits) - 1, (nbit + 63) // 64
    c = rng.standard_normal((Qn, nbit)).astype(np.float32)
    c[3] = 0.0                                                      # amax = 0: every weight 0
    c[4, 1], c[4, 7], c[4, nbit - 1] = np.nan, np.inf, -np.inf      # not finite: weight 0, and not the maximum
    c[5] = 0.0                                                      # a / amax = (m + 0.5) / L exactly: rounds up, in fp64 and nowhere else
    c[5, 0] = L
    c[5, 1:1 + min(L, nbit - 1)] = (np.arange(min(L, nbit - 1)) + 0.5) * np.where(np.arange(min(L, nbit - 1)) % 2, -1, 1)
    c[6] = np.float32(1e-30) * rng.standard_normal(nbit)            # tiny and huge rows: the quotient is scale free
    c[7] = np.float32(1e30) * rng.standard_normal(nbit)
    c[8, :] = -0.0
    per = _mask_words(rng, Qn, nbit)
    per[9] = 0                                                      # a mask that clears every bit
    per[10] = ~ref.pack_bits((np.abs(np.pad(c[10], (0, 64 * W - nbit))) == np.abs(c[10]).max())[None, :])[0]   # ... or just the row's maximum
    shared = per[11].copy()
    t = _t(c, dev)
    for mask in (None, shared, per):
        w = ref.weights(c, bits, mask)
        planes, wsum = rt.weight_planes(t, bits, None if mask is None else _t(mask, dev))
        assert planes.shape == (Qn, bits, W) and planes.dtype == torch.int64 and wsum.shape == (Qn,) and wsum.dtype == torch.int32
        got = _u64(planes)
        assert np.array_equal(got, ref.planes_of(w, bits)), (nbit, bits, None if mask is None else mask.ndim)
        assert np.array_equal(wsum.cpu().numpy(), w.sum(1))
        if nbit % 64:                                               # bits past nbit are clear in every plane
            assert not (got[:, :, -1] >> np.uint64(nbit % 64)).any()
        assert not got[3].any() and not got[8].any() and (mask is None or mask.ndim == 1 or not got[9].any())
    w = ref.weights(c, bits)
    assert w[5, 0] == L and w[5, 1:4].tolist() == [1, 2, 3] and w[4, 1] == w[4, 7] == w[4, nbit - 1] == 0 and w[4].max() == L
    assert w[6].max() == L and w[7].max() == L
    with pytest.raises(ValueError):
        rt.weight_planes(t, 5)
    with pytest.raises(ValueError):
        rt.weight_planes(t, bits, _t(per[:5], dev))
    planes, wsum = rt.weight_planes(t[:0], bits)
    assert planes.shape == (0, bits, W) and wsum.shape == (0,)


# ---- the scan ----------------------------------------------------------------------------------------------------------------------

def _tied_problem(W, seed=0):
    """|c| in {0.25, 0.5, 1} with random signs, 200 random gallery rows repeated to 771: every row is there 3-4 times, and three weight
    levels leave many different rows at one distance"""
    rng = np.random.default_rng(50 + W + seed)
    nbit = 64 * W
    c = (rng.choice(np.array([0.25, 0.5, 1.0], np.float32), (QN_TIES, nbit)) * rng.choice(np.array([-1.0, 1.0], np.float32), (QN_TIES, nbit)))
    g = ref.pack_sign(rng.standard_normal((200, nbit)).astype(np.float32))
    g = np.tile(g, (4, 1))[:G_TIES]
    return c.astype(np.float32), g


_TIED = {}


def _tied(W, bits):
    """the reference of one (W, bits), computed once and shared by the cases of the tests below; never modified"""
    if (W, bits) not in _TIED:
        c, g = _tied_problem(W)
        q = ref.pack_sign(c)
        w = ref.weights(c, bits)
        D = ref.dist(q, g, w)
        D.setflags(write=False)
        _TIED[(W, bits)] = (c, q, g, w, D)
    return _TIED[(W, bits)]


@pytest.mark.parametrize("k", [1, 10, 16, 17, 128])          # KREG 10, 10, 16, 32, 128 (64: the edge test)
@pytest.mark.parametrize("W", [1, 2, 3, 4])
@pytest.mark.parametrize("bits", [4, 8])
def test_weighted_topk_orders_engineered_ties_by_gallery_index(dev, W, bits, k):
    from concepthash_amd import retrieval as rt
    c, q, g, w, D = _tied(W, bits)
    tied = ref.tied_at_k(D, 10)
    print(f"W = {W}, {bits}-bit weights: {tied:.1%} of the queries tie at k = 10")
    assert tied >= 0.5, f"vacuous: only {tied:.1%} of the queries have a left-out row tied with their 10th hit"
    t = _t(c, dev)
    planes, wsum = rt.weight_planes(t, bits)
    assert np.array_equal(_u64(planes), ref.planes_of(w, bits)) and np.array_equal(wsum.cpu().numpy(), w.sum(1))
    gq, gg = rt.pack_sign(t), _t(g, dev)
    assert np.array_equal(_u64(gq), q)
    got = rt.hamming_topk_weighted(gq, planes, gg, k)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32
    assert _same(got, ref.topk(D, k)), (W, bits, k)


@pytest.mark.parametrize("bits", [4, 8])
def test_weighted_topk_gallery_and_query_edges(dev, bits):
    """continuous codes (no ties): the -1 fill, segment tails of 1, 2 and 3 rows, a ragged last query tile, g_index_base"""
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(7 + bits)
    nbit, W = 120, 2
    c = rng.standard_normal((300, nbit)).astype(np.float32)
    g = ref.pack_sign(rng.standard_normal((1030, nbit)).astype(np.float32))
    q, w = ref.pack_sign(c), ref.weights(c, bits)
    D = ref.dist(q, g, w)
    t, gg = _t(c, dev), _t(g, dev)
    planes, _ = rt.weight_planes(t, bits)
    gq = rt.pack_sign(t)
    for G in (0, 5, 257, 258, 259, 1030):
        got = rt.hamming_topk_weighted(gq[:65], planes[:65], gg[:G], 10, g_index_base=1000)
        want = ref.topk(D[:65, :G], 10, 1000)
        assert _same(got, want), G
        assert G >= 10 or ((want[0][:, G:] == -1).all() and (want[1][:, G:] == -1).all())
    for Qn in (1, 65, 300):
        assert _same(rt.hamming_topk_weighted(gq[:Qn], planes[:Qn], gg, 10), ref.topk(D[:Qn], 10)), Qn
    assert _same(rt.hamming_topk_weighted(gq[:65], planes[:65], gg, 64, g_index_base=1000), ref.topk(D[:65], 64, 1000))   # KREG 64
    idx, dst = rt.hamming_topk_weighted(gq[:0], planes[:0], gg, 3)
    assert idx.shape == (0, 3) and dst.shape == (0, 3)
    with pytest.raises(ValueError):
        rt.hamming_topk_weighted(gq, planes[:5], gg, 3)
    with pytest.raises(ValueError):
        rt.hamming_topk_weighted(gq, planes[:, :3], gg, 3)


@pytest.mark.parametrize("W", [1, 2, 4])
@pytest.mark.parametrize("bits", [4, 8])
def test_weighted_topk_with_unit_codes_is_the_hamming_ranking(dev, W, bits):
    """codes in {-1, +1}: every weight is L, so D = L * hamming and the ranking is hamming_topk's; with a per-query mask, hamming_topk_masked's"""
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(90 + W)
    nbit, L = 64 * W - (16 if W == 1 else 0), (1 << bits) - 1
    c = rng.choice(np.array([-1.0, 1.0], np.float32), (130, nbit))
    g = ref.pack_sign(rng.standard_normal((301, nbit)).astype(np.float32))
    t, gg = _t(c, dev), _t(g, dev)
    gq = rt.pack_sign(t)
    planes, wsum = rt.weight_planes(t, bits)
    assert (wsum == L * nbit).all()
    for k in (10, 32):
        idx, dst = rt.hamming_topk_weighted(gq, planes, gg, k, g_index_base=9)
        hidx, hdst = rt.hamming_topk(gq, gg, k, g_index_base=9)
        assert torch.equal(idx, hidx) and torch.equal(dst, L * hdst)
    mask = _t(_mask_words(rng, 130, nbit), dev)
    planes, wsum = rt.weight_planes(t, bits, mask)
    idx, dst = rt.hamming_topk_weighted(gq, planes, gg, 10)
    midx, mdst = rt.hamming_topk_masked(gq, gg, mask, 10)           # (the codes are zero past nbit: the mask's bits there count nothing)
    assert torch.equal(idx, midx) and torch.equal(dst, L * mdst)


@pytest.mark.parametrize("bits", [4, 8])
def test_weighted_topk_of_ragged_shards_merges_to_the_single_call(dev, bits):
    from concepthash_amd import retrieval as rt
    c, q, g, w, D = _tied(2, bits)
    t, gg = _t(c, dev), _t(g, dev)
    gq = rt.pack_sign(t)
    planes, _ = rt.weight_planes(t, bits)
    for k in (10, 40):
        whole = rt.hamming_topk_weighted(gq, planes, gg, k)
        assert _same(whole, ref.topk(D, k))
        cuts = (0, 5, 300, G_TIES)
        parts = [rt.hamming_topk_weighted(gq, planes, gg[a:b], k, g_index_base=a) for a, b in zip(cuts[:-1], cuts[1:])]
        merged = rt.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
        assert torch.equal(merged[0], whole[0]) and torch.equal(merged[1], whole[1])


# ---- the index ---------------------------------------------------------------------------------------------------------------------

def test_gallery_index_search_ranks_by_the_asymmetric_distance(dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    rng = np.random.default_rng(21)
    nbit, Q, G, Qn, k = 120, 3, 301, 70, 10
    db = rng.standard_normal((G, nbit)).astype(np.float32)
    qc = rng.standard_normal((Qn, nbit)).astype(np.float32)
    mean = db.mean(0)
    labels = torch.from_numpy(rng.integers(0, 9, G))
    index = GalleryIndex(rt.pack_sign(_t(db - mean, dev)), nbit, Q, labels=labels, paths=[f"img/{i}.jpg" for i in range(G)], data_root="/d",
                         mean=torch.from_numpy(mean)).to(dev)
    tq = _t(qc, dev)
    centred = tq - _t(mean, dev)[None, :]
    gq = rt.pack_sign(centred)
    for concepts, margin in (([0, 2], 0.3), (None, 0.0), ([1], 0.0), (None, 0.3)):
        for bits in (8, 4):
            res = index.search(tq, k, concepts, margin, rank="asymmetric", weight_bits=bits)
            mask = None
            if concepts is not None:
                mask = rt.concept_mask(nbit, Q, concepts).to(dev)
            if margin > 0:
                conf = rt.confidence_mask(centred, margin)
                mask = conf if mask is None else conf & mask[None, :]
            planes, wsum = rt.weight_planes(centred, bits, mask)
            idx, dst = rt.hamming_topk_weighted(gq, planes, index.codes, k)
            assert torch.equal(res["idx"], idx) and torch.equal(res["dist"], dst) and torch.equal(res["dist_max"], wsum)
            assert res["rank"] == "asymmetric" and res["weight_bits"] == bits
            # ... and the numpy reference on the same centred codes, with the mask of the Hamming ranking
            cn = centred.cpu().numpy()
            w = ref.weights(cn, bits, None if mask is None else _u64(mask))
            assert _same((idx, dst), ref.topk(ref.dist(ref.pack_sign(cn), _u64(index.codes), w), k)), (concepts, margin, bits)
            ham = index.search(tq, k, concepts, margin)
            assert torch.equal(res["bits"], ham["bits"])
            assert torch.equal(res["concept_dist"], rt.subcode_dist(gq, index.codes, idx, nbit, Q))      # unmasked and unweighted, on these hits' rows
            assert np.array_equal(res["labels"].cpu().numpy(), labels.numpy()[idx.cpu().numpy()])
            assert res["paths"][3][0] == f"img/{int(idx[3, 0])}.jpg"
        # rank="hamming" is the call without the new arguments, key for key
        ham = index.search(tq, k, concepts, margin)
        named = index.search(tq, k, concepts, margin, rank="hamming", weight_bits=4)
        assert set(named) == set(ham) == {"idx", "dist", "concept_dist", "bits", "labels", "paths"}
        assert all(torch.equal(named[n], ham[n]) for n in ("idx", "dist", "concept_dist", "bits", "labels")) and named["paths"] == ham["paths"]


# ---- the command -------------------------------------------------------------------------------------------------------------------

COMMON = ["dataset=synthetic_cub200", "dataset.limit=96", "batch_size=32"]


def _main_v2(args, cwd):
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py")] + args, check=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=cwd,
                   timeout=600)


def test_search_command_ranks_by_the_asymmetric_distance(tmp_path, dev):
    """a synthetic run directory, built as tests/test_search_gpu.py builds its own; the evaluator's saved codes are the queries"""
    from concepthash_amd.search import GalleryIndex
    tmp = tmp_path
    logdir = str(tmp / "run")
    common = COMMON + ["data_dir=" + str(tmp)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp))
    ev, s1, s2 = str(tmp / "ev"), str(tmp / "s1"), str(tmp / "s2")
    _main_v2(["--config-name", "val.yaml", "logdir=" + logdir, "save_code=True", "eval_logdir=" + ev] + common, str(tmp))
    _main_v2(["--config-name", "search.yaml", "logdir=" + logdir, "search_logdir=" + s1, "rank=asymmetric", "weight_bits=4", "concepts=[0,3]",
              "k=7"] + common, str(tmp))
    _main_v2(["--config-name", "search.yaml", "logdir=" + logdir, "search_logdir=" + s2] + common, str(tmp))
    te = torch.load(os.path.join(ev, "outputs.pth"))["test"]["codes"].to(dev)
    index = GalleryIndex.load(os.path.join(logdir, "index_best.pth")).to(dev)
    res = json.load(open(os.path.join(s1, "results.json")))
    assert res["rank"] == "asymmetric" and res["weight_bits"] == 4 and res["k"] == 7 and res["concepts"] == [0, 3]
    want = index.search(te, 7, [0, 3], 0.0, rank="asymmetric", weight_bits=4)
    idx, dst, dmax = want["idx"].tolist(), want["dist"].tolist(), want["dist_max"].tolist()
    assert len(res["queries"]) == 96
    for i, e in enumerate(res["queries"]):
        assert e["unmasked_bits"] == 32 and e["distance_max"] == dmax[i] and 15 <= dmax[i] <= 15 * 32
        assert [h["index"] for h in e["hits"]] == idx[i] and [h["distance"] for h in e["hits"]] == dst[i], i
        assert all(0 <= h["distance"] <= dmax[i] and len(h["concept_distances"]) == 4 for h in e["hits"])
    # the default ranking: today's values, plus the three new keys
    res = json.load(open(os.path.join(s2, "results.json")))
    assert res["rank"] == "hamming" and res["weight_bits"] == 8 and res["k"] == 10 and res["concepts"] is None
    assert res["index_status"] == "loaded"
    ham = index.search(te, 10)
    idx, dst = ham["idx"].tolist(), ham["dist"].tolist()
    for i, e in enumerate(res["queries"]):
        assert set(e) == {"query", "label", "unmasked_bits", "distance_max", "hits"} and e["unmasked_bits"] == e["distance_max"] == 64
        assert [h["index"] for h in e["hits"]] == idx[i] and [h["distance"] for h in e["hits"]] == dst[i], i
        assert all(sum(h["concept_distances"]) == h["distance"] for h in e["hits"])
