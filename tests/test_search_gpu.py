"""GPU: the search feature.  Masked top-k (ch_hamming_topk_masked) and the per-sub-code breakdown (ch_hamming_subcode_dist) against
numpy -- `np.unpackbits` of the masked XOR, a stable sort by distance, i.e. ascending (distance, index) -- at the smallest shapes that
reach every path of the kernels; then `main_v2.py --config-name search.yaml` on a synthetic run directory and on JPEG files, and the
evaluator's per-concept table.  All arithmetic is integer: every comparison is exact."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import weighted_topk_ref as wref
from conftest import ROOT

pytestmark = pytest.mark.gpu

G_TWO_SEGMENTS = 301      # topk_seg_rows gives 256-row segments: 256 + 45 rows = five double blocks, one single block, a one-row tail
QNS = (1, 70, 257)        # one lane; a partial wave; a second query tile with one live lane
KS = (1, 10, 16, 32, 64, 128)   # every KREG instantiation (10, 10, 16, 32, 64, 128)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _codes(rng, rows, nbit):
    """random packed codes [rows, W] uint64 with the bits past nbit zero (as pack_sign leaves them)"""
    W = (nbit + 63) // 64
    a = rng.integers(0, 1 << 63, (rows, W), dtype=np.uint64) ^ (rng.integers(0, 2, (rows, W), dtype=np.uint64) << np.uint64(63))
    if nbit % 64:
        a[:, -1] &= np.uint64((1 << (nbit % 64)) - 1)
    return a


def _bits(x):
    """[..., W] uint64 -> [..., 64 W] {0,1}, bit i of word w at position 64 w + i"""
    x = np.ascontiguousarray(x)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape[:-1] + (x.shape[-1] * 8,)), axis=-1, bitorder="little")


def _ref_dist(q, g, mask=None):
    """[Qn, G] popcount((q ^ g) & mask); mask [W], [Qn, W] or None"""
    x = q[:, None, :] ^ g[None, :, :]
    if mask is not None:
        x = x & (mask[None, None, :] if mask.ndim == 1 else mask[:, None, :])
    return _bits(x).sum(-1, dtype=np.int32)


def _ref_topk(d, k, base=0):
    """ascending (distance, index) from a distance matrix; -1 past the end of the gallery"""
    Qn, G = d.shape
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    idx = np.full((Qn, k), -1, np.int64)
    dst = np.full((Qn, k), -1, np.int32)
    idx[:, :order.shape[1]] = order + base
    dst[:, :order.shape[1]] = np.take_along_axis(d, order, 1)
    return idx, dst


def _same(got, want):
    return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


# ---- masked top-k ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_masked_topk_equals_numpy_on_every_code_path(dev, W):
    from concepthash_amd import retrieval as rt
    nbit = 48 if W == 1 else 64 * W
    rng = np.random.default_rng(100 + W)
    q, g = _codes(rng, max(QNS), nbit), _codes(rng, G_TWO_SEGMENTS, nbit)
    per_query = rng.integers(0, 1 << 63, (max(QNS), W), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (max(QNS), W), dtype=np.uint64)
    shared = per_query[5].copy()
    if W == 1:    # the 16 unused high bits: zero in the codes, SET in the masks -- they must not count
        per_query |= np.uint64(0xFFFF << 48)
        shared |= np.uint64(0xFFFF << 48)
    assert (per_query[:-1] != per_query[1:]).any(1).all()          # neighbouring lanes hold different masks
    gq, gg = _t(q, dev), _t(g, dev)
    for mask, name in ((per_query, "per-query"), (shared, "shared")):
        d = _ref_dist(q, g, mask)                                   # once per mask kind, for all 257 queries
        gm = _t(mask, dev)
        for Qn in QNS:
            for k in KS:
                base = 0 if k == 10 else 1000 * k + Qn              # a non-zero g_index_base everywhere but one k
                got = rt.hamming_topk_masked(gq[:Qn], gg, gm[:Qn] if mask.ndim == 2 else gm, k, g_index_base=base)
                assert _same(got, _ref_topk(d[:Qn], k, base)), (name, Qn, k)
    # for shared masks the CPU oracle on pre-masked codes does the same job
    from oracle import hamming_oracle as ho
    oidx, odst = ho.topk(q & shared, g & shared, 10)
    got = rt.hamming_topk_masked(gq, gg, _t(shared, dev), 10)
    assert np.array_equal(got[0].cpu().numpy(), oidx.astype(np.int64)) and np.array_equal(got[1].cpu().numpy(), odst)


def test_masked_topk_short_and_empty_galleries(dev):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(7)
    q, g = _codes(rng, 70, 128), _codes(rng, 7, 128)
    mask = _codes(rng, 70, 128)
    got = rt.hamming_topk_masked(_t(q, dev), _t(g, dev), _t(mask, dev), 10, g_index_base=50)        # k > G: the tail is -1
    want = _ref_topk(_ref_dist(q, g, mask), 10, 50)
    assert _same(got, want) and (want[0][:, 7:] == -1).all() and (want[1][:, 7:] == -1).all()
    for m in (mask, mask[0]):                                                                        # G = 0
        idx, dst = rt.hamming_topk_masked(_t(q, dev), _t(g[:0], dev), _t(m, dev), 3)
        assert idx.shape == (70, 3) and (idx.cpu().numpy() == -1).all() and (dst.cpu().numpy() == -1).all()
    idx, dst = rt.hamming_topk_masked(_t(q[:0], dev), _t(g, dev), _t(mask[0], dev), 3)               # no queries
    assert idx.shape == (0, 3) and dst.shape == (0, 3)
    with pytest.raises(ValueError):
        rt.hamming_topk_masked(_t(q, dev), _t(g, dev), _t(mask[:5], dev), 3)                         # neither [W] nor [Qn, W]


@pytest.mark.parametrize("W", [1, 2, 4])
def test_masked_topk_identity_masks(dev, W):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(40 + W)
    q, g = _codes(rng, 257, 64 * W), _codes(rng, G_TWO_SEGMENTS, 64 * W)
    gq, gg = _t(q, dev), _t(g, dev)
    for k in (10, 32, 128):
        plain = rt.hamming_topk(gq, gg, k, g_index_base=9)
        for ones in (torch.full((W,), -1, dtype=torch.int64, device=dev), torch.full((257, W), -1, dtype=torch.int64, device=dev)):
            got = rt.hamming_topk_masked(gq, gg, ones, k, g_index_base=9)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        for zeros in (torch.zeros(W, dtype=torch.int64, device=dev), torch.zeros(257, W, dtype=torch.int64, device=dev)):
            idx, dst = rt.hamming_topk_masked(gq, gg, zeros, k, g_index_base=9)
            assert (dst == 0).all() and torch.equal(idx, (9 + torch.arange(k, device=dev))[None, :].expand(257, k))


def test_masked_topk_orders_heavy_ties_by_gallery_index(dev):
    """codes that differ in three bits only: the distances are 0..3, nearly every row ties, and the order inside a distance must be
    the gallery index -- across the two segments and through the merge"""
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(3)
    spread = np.array([1 << 3, 1 << 40, 1 << 63], dtype=np.uint64)

    def three_bit(rows):
        return (rng.integers(0, 2, (rows, 3)).astype(np.uint64) * spread).sum(1, dtype=np.uint64)[:, None]
    q, g = three_bit(130), three_bit(G_TWO_SEGMENTS)
    per_query = np.where(rng.integers(0, 4, (130, 1)) == 0, np.uint64(1 << 40 | 1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF))
    for mask in (per_query, np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64), np.array([1 << 3 | 1 << 63], dtype=np.uint64)):
        d = _ref_dist(q, g, mask)
        assert len(np.unique(d)) in (3, 4)
        for k in (10, 40, 128):
            assert _same(rt.hamming_topk_masked(_t(q, dev), _t(g, dev), _t(mask, dev), k), _ref_topk(d, k)), k


# ---- the scan body the three distances share ---------------------------------------------------------------------------------------

SCAN_EXIT_G = tuple(base + g for base in (0, 256) for g in (1, 3, 4, 5, 8, 11, 12, 13))


@pytest.mark.parametrize("W", [1, 3])
def test_scan_exits_agree_for_plain_masked_and_weighted(dev, W):
    """topk_scan's ways out of a segment, for the three distances at once: segments of 1 and 3 rows (no whole four-row block), 4 and 5
    (one: the odd-block exit), 8 and 11 (two), 12 and 13 (three), i.e. remainders of 0, 1 and 3 rows after none, an odd and an even
    number of whole blocks; with 256 more rows the same tails follow a full segment of 64 blocks (segments hold 256 rows at these
    sizes) and the merge joins the two.  70 queries leave lanes past Qn in the second wave.  (distance, index) exactly."""
    from concepthash_amd import retrieval as rt
    nbit, Qn, k, Gmax = 64 * W, 70, 10, max(SCAN_EXIT_G)
    rng = np.random.default_rng(700 + W)
    c = rng.standard_normal((Qn, nbit)).astype(np.float32)
    q, g = wref.pack_sign(c), _codes(rng, Gmax, nbit)
    mask = _codes(rng, Qn, nbit)
    t, gq, gg, gm = _t(c, dev), _t(q, dev), _t(g, dev), _t(mask, dev)
    assert np.array_equal(rt.pack_sign(t).cpu().numpy().view(np.uint64), q)
    d_plain, d_masked = _ref_dist(q, g), _ref_dist(q, g, mask)          # once, for the longest gallery: a row's distance is its own
    weighted = {}
    for bits in (4, 8):
        w = wref.weights(c, bits)
        planes, _ = rt.weight_planes(t, bits)
        assert np.array_equal(planes.cpu().numpy().view(np.uint64), wref.planes_of(w, bits))
        weighted[bits] = (planes, wref.dist(q, g, w))
    for G in SCAN_EXIT_G:
        assert _same(rt.hamming_topk(gq, gg[:G], k), _ref_topk(d_plain[:, :G], k)), ("plain", G)
        assert _same(rt.hamming_topk_masked(gq, gg[:G], gm, k), _ref_topk(d_masked[:, :G], k)), ("masked", G)
        for bits, (planes, D) in weighted.items():
            assert _same(rt.hamming_topk_weighted(gq, planes, gg[:G], k), wref.topk(D[:, :G], k)), (bits, G)


# ---- per-sub-code distances --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbit,nsub", [(64, 4), (48, 4), (120, 3), (256, 4), (64, 1)])
def test_subcode_dist_equals_the_per_slice_popcounts(dev, nbit, nsub):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(nbit + nsub)
    q, g = _codes(rng, 70, nbit), _codes(rng, G_TWO_SEGMENTS, nbit)
    gq, gg = _t(q, dev), _t(g, dev)
    base = 12345
    idx, dst = rt.hamming_topk(gq, gg, 10, g_index_base=base)
    got = rt.subcode_dist(gq, gg, idx, nbit, nsub, g_index_base=base)
    assert got.shape == (70, 10, nsub) and got.dtype == torch.int32
    rows = idx.cpu().numpy() - base
    x = _bits(q[:, None, :] ^ g[rows])[..., :nbit]                                   # [Qn, k, nbit]
    want = x.reshape(70, 10, nsub, nbit // nsub).sum(-1, dtype=np.int32)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got.sum(-1, dtype=torch.int32), dst)                          # the sub-codes add up to the whole-code distance
    # a short gallery: the -1 hits give -1 rows, the others their popcounts
    idx7, dst7 = rt.hamming_topk(gq, gg[:7], 10, g_index_base=base)
    got7 = rt.subcode_dist(gq, gg[:7], idx7, nbit, nsub, g_index_base=base).cpu().numpy()
    assert (got7[:, 7:] == -1).all() and np.array_equal(got7[:, :7].sum(-1), dst7.cpu().numpy()[:, :7])
    # an index outside [base, base + G) is refused on the host, before any row is read through it
    for bad in (base + G_TWO_SEGMENTS, base - 1, -2):
        wrong = idx.clone()
        wrong[3, 4] = bad
        with pytest.raises(RuntimeError, match="idx"):
            rt.subcode_dist(gq, gg, wrong, nbit, nsub, g_index_base=base)
    with pytest.raises(RuntimeError, match="idx"):
        rt.subcode_dist(gq, gg, idx, nbit, nsub, g_index_base=0)                     # the base of another shard


# ---- masks -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbit", [16, 48, 64, 120, 256])
def test_confidence_mask_is_the_packed_magnitude_test(dev, nbit):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(nbit)
    margin = 0.3
    codes = rng.standard_normal((257, nbit)).astype(np.float32)
    codes[::3, ::5] = np.float32(margin)            # entries exactly at +-margin are NOT above it
    codes[1::3, 1::5] = -np.float32(margin)
    codes[2, :] = 0.0
    t = _t(codes, dev)
    got = rt.confidence_mask(t, margin).cpu().numpy().view(np.uint64)
    keep = (t.abs() > margin).cpu().numpy()
    assert np.array_equal(keep, np.abs(codes) > np.float32(margin))
    W = (nbit + 63) // 64
    padded = np.zeros((257, 64 * W), np.uint8)
    padded[:, :nbit] = keep
    want = np.packbits(padded, axis=-1, bitorder="little").view(np.uint64)
    assert got.shape == (257, W) and np.array_equal(got, want)
    assert not keep[::3, ::5].any() and not keep[1::3, 1::5].any() and not keep[2].any()


def test_gallery_index_search_combines_concepts_and_margin(dev):
    """GalleryIndex.search: the mean is subtracted from the queries, `concepts` is a shared mask, `margin` a per-query one, both = their AND"""
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    rng = np.random.default_rng(11)
    nbit, Q, G, Qn, k = 120, 3, G_TWO_SEGMENTS, 70, 10
    db = rng.standard_normal((G, nbit)).astype(np.float32)
    qc = rng.standard_normal((Qn, nbit)).astype(np.float32)
    mean = db.mean(0)
    labels = torch.from_numpy(rng.integers(0, 9, G))
    index = GalleryIndex(rt.pack_sign(_t(db - mean, dev)), nbit, Q, labels=labels, paths=[f"img/{i}.jpg" for i in range(G)], data_root="/d",
                         mean=torch.from_numpy(mean)).to(dev)
    centred = qc - mean
    diff = (centred[:, None, :] > 0) != ((db - mean)[None, :, :] > 0)                # [Qn, G, nbit]
    for concepts, margin in ((None, 0.0), ([0, 2], 0.0), (None, 0.4), ([1], 0.4), ([2, 0, 1], 0.0)):
        keep = np.ones((Qn, nbit), bool)
        if concepts is not None:
            cols = np.zeros(nbit, bool)
            for c in concepts:
                cols[c * 40:(c + 1) * 40] = True
            keep &= cols
        if margin > 0:
            keep &= np.abs(centred) > np.float32(margin)
        d = (diff & keep[:, None, :]).sum(-1, dtype=np.int32)
        res = index.search(_t(qc, dev), k, concepts, margin)
        want = _ref_topk(d, k)
        assert _same((res["idx"], res["dist"]), want), (concepts, margin)
        assert np.array_equal(res["bits"].cpu().numpy(), keep.sum(1))
        per_concept = diff[np.arange(Qn)[:, None], want[0]].reshape(Qn, k, Q, 40).sum(-1)           # unmasked, whatever the ranking mask
        assert np.array_equal(res["concept_dist"].cpu().numpy(), per_concept)
        assert np.array_equal(res["labels"].cpu().numpy(), labels.numpy()[want[0]])
        assert res["paths"][3][0] == f"img/{want[0][3, 0]}.jpg"


# ---- the command -------------------------------------------------------------------------------------------------------------------

COMMON = ["dataset=synthetic_cub200", "dataset.limit=96", "batch_size=32"]


def _main_v2(args, cwd):
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py")] + args, check=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=cwd,
                   timeout=600)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One synthetic run directory, the evaluator's saved codes of it (`outputs.pth`, the file `exp=extract` writes -- written here by
    the checkpoint-loading `val.yaml` command with save_code, because `exp=extract` encodes with a freshly built model, not with the
    run's checkpoint) with the per-concept table, and the first search: shared by the tests below."""
    tmp = tmp_path_factory.mktemp("search")
    logdir = str(tmp / "run")
    common = COMMON + ["data_dir=" + str(tmp)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp))
    ev = str(tmp / "ev")
    _main_v2(["--config-name", "val.yaml", "logdir=" + logdir, "save_code=True", "concept_eval=true", "eval_logdir=" + ev] + common, str(tmp))
    s1 = str(tmp / "s1")
    _main_v2(["--config-name", "search.yaml", "logdir=" + logdir, "search_logdir=" + s1] + common, str(tmp))
    outs = torch.load(os.path.join(ev, "outputs.pth"))
    return dict(tmp=tmp, logdir=logdir, common=common, outs=outs, history=json.load(open(os.path.join(ev, "history.json"))),
                first=json.load(open(os.path.join(s1, "results.json"))))


def test_search_hits_equal_topk_on_the_evaluators_codes(run, dev):
    from concepthash_amd import retrieval as rt
    te, db = run["outs"]["test"], run["outs"]["db"]
    assert te["codes"].shape == (96, 64) and db["codes"].shape == (96, 64)
    q, g = rt.pack_sign(te["codes"].to(dev)), rt.pack_sign(db["codes"].to(dev))
    idx, dst = rt.hamming_topk(q, g, 10)
    idx, dst = idx.cpu().tolist(), dst.cpu().tolist()
    res = run["first"]
    assert res["k"] == 10 and res["concepts"] is None and res["query_margin"] == 0.0 and res["index_rows"] == 96
    assert res["index"] == os.path.join(run["logdir"], "index_best.pth") and os.path.exists(res["index"])
    assert res["index_status"].startswith("built") and "encode_db" in res["timing_s"] and "encode_query" in res["timing_s"]
    ql, gl = te["labels"].argmax(1).tolist(), db["labels"].argmax(1).tolist()
    assert len(res["queries"]) == 96
    for i, e in enumerate(res["queries"]):
        assert e["query"] == i and e["label"] == ql[i] and e["unmasked_bits"] == 64
        assert [h["index"] for h in e["hits"]] == idx[i] and [h["distance"] for h in e["hits"]] == dst[i], i
        for r, h in enumerate(e["hits"]):
            assert h["rank"] == r + 1 and h["path"] is None and h["label"] == gl[h["index"]] and h["relevant"] == (gl[h["index"]] == ql[i])
            assert len(h["concept_distances"]) == 4 and sum(h["concept_distances"]) == h["distance"]


def test_second_search_loads_the_index_and_ranks_by_one_concept(run):
    s2 = str(run["tmp"] / "s2")
    _main_v2(["--config-name", "search.yaml", "logdir=" + run["logdir"], "search_logdir=" + s2, "concepts=[1]", "k=7"] + run["common"],
             str(run["tmp"]))
    res = json.load(open(os.path.join(s2, "results.json")))
    # the cached index: found, matched to the checkpoint, and the database split not encoded again
    assert res["index_status"] == "loaded" and "index_load" in res["timing_s"] and "encode_db" not in res["timing_s"]
    assert res["concepts"] == [1] and res["k"] == 7
    te, db = run["outs"]["test"]["codes"].numpy(), run["outs"]["db"]["codes"].numpy()
    d = ((te[:, None, 16:32] > 0) != (db[None, :, 16:32] > 0)).sum(-1, dtype=np.int32)      # Hamming distance of columns [16, 32)
    widx, wdst = _ref_topk(d, 7)
    whole = ((te[:, None, :] > 0) != (db[None, :, :] > 0)).reshape(96, 96, 4, 16).sum(-1)
    for i, e in enumerate(res["queries"]):
        assert e["unmasked_bits"] == 16
        assert [h["index"] for h in e["hits"]] == widx[i].tolist() and [h["distance"] for h in e["hits"]] == wdst[i].tolist(), i
        for h in e["hits"]:
            assert h["concept_distances"] == whole[i, h["index"]].tolist() and h["concept_distances"][1] == h["distance"]


def test_concept_eval_table_equals_separate_sub_code_evaluations(run):
    hist = run["history"]
    assert len(hist["mAP_concept"]) == len(hist["recalls_concept"]) == len(hist["precisions_concept"]) == 4
    assert all(len(r) == 3 for r in hist["recalls_concept"]) and all(len(p) == 3 for p in hist["precisions_concept"])
    for c in (0, 2):
        ev = str(run["tmp"] / f"sub{c}")
        _main_v2(["--config-name", "val.yaml", "logdir=" + run["logdir"], "eval_logdir=" + ev, "sub_code_eval=True",
                  f"sub_code_eval_setting.start_bit={16 * c}", f"sub_code_eval_setting.end_bit={16 * c + 16}",
                  "sub_code_eval_setting.rand_bits=1"] + run["common"], str(run["tmp"]))
        sub = json.load(open(os.path.join(ev, "history.json")))
        assert "mAP_concept" not in sub                                  # the key is off by default: nothing is added
        assert hist["mAP_concept"][c] == sub["mAP"] and hist["precisions_concept"][c] == sub["precisions"] \
            and hist["recalls_concept"][c] == sub["recalls"], c


def test_search_on_jpeg_files_finds_each_query_file_itself(run):
    from test_preprocess import _write_dataset
    tmp = run["tmp"] / "jpeg"
    data = tmp / "data" / "cub200_2011"
    data.mkdir(parents=True)
    _write_dataset(str(data), [(300, 400), (400, 300), (300, 300), (250, 330), (280, 280), (320, 260), (260, 390), (310, 310)])
    lines = open(data / "train.txt").read()
    for name in ("test.txt", "database.txt"):
        (data / name).write_text(lines)
    args = ["--config-name", "search.yaml", "logdir=" + run["logdir"], "dataset=cub200", "data_dir=" + str(tmp), "batch_size=32", "k=5",
            "index=" + str(tmp / "jpeg_index.pth")]
    # a single image path; it builds the index.  Database row 0 has no row in front of it, so whatever the codes it ranks itself first
    one = str(tmp / "one")
    _main_v2(args + ["query=" + str(data / "img" / "0.jpg"), "search_logdir=" + one], str(tmp))
    res = json.load(open(os.path.join(one, "results.json")))
    assert res["index"] == str(tmp / "jpeg_index.pth") and res["index_status"].startswith("built") and res["index_rows"] == 8
    assert len(res["queries"]) == 1 and res["queries"][0]["query"] == str(data / "img" / "0.jpg") and res["queries"][0]["label"] is None
    top = res["queries"][0]["hits"][0]
    assert top["distance"] == 0 and top["index"] == 0 and os.path.samefile(top["path"], data / "img" / "0.jpg") and top["label"] == 0
    # The directory's three files.  The ranking is ascending (distance, index), so a file is its own rank-1 hit exactly when no EARLIER
    # database row holds the same code (the seeded random checkpoint gives some of these pictures equal codes): the queries are the
    # first three database files with that property, read off the encoder's packed codes in the index file -- not off any ranking.
    from concepthash_amd.search import GalleryIndex
    index = GalleryIndex.load(str(tmp / "jpeg_index.pth"))
    assert index.paths == [f"img/{i}.jpg" for i in range(8)] and index.data_root == str(data) and index.labels.tolist() == [i % 5 for i in range(8)]
    assert index.transform == {"resize": 256, "crop": 224, "norm": 2} and index.mean is None and (index.nbit, index.ncontext) == (64, 4)
    seen, first = set(), []
    for i, code in enumerate(index.codes.tolist()):
        if tuple(code) not in seen:
            first.append(i)
        seen.add(tuple(code))
    assert len(first) >= 3, first
    picked = sorted(f"{i}.jpg" for i in first[:3])
    qdir = tmp / "queries"
    qdir.mkdir()
    for name in picked:
        shutil.copy(data / "img" / name, qdir / name)
    (qdir / "notes.txt").write_text("not an image")
    (qdir / "nested").mkdir()
    shutil.copy(data / "img" / "1.jpg", qdir / "nested" / "1.jpg")               # not recursive
    out = str(tmp / "s")
    _main_v2(args + ["query=" + str(qdir), "save_attention=true", "search_logdir=" + out], str(tmp))
    res = json.load(open(os.path.join(out, "results.json")))
    assert res["index_status"] == "loaded" and "encode_db" not in res["timing_s"]
    assert [os.path.basename(e["query"]) for e in res["queries"]] == picked
    for e, name in zip(res["queries"], picked):
        assert e["label"] is None and len(e["hits"]) == 5
        top = e["hits"][0]
        assert top["distance"] == 0 and os.path.basename(top["path"]) == name and top["label"] == int(name[0]) % 5, e
        assert open(top["path"], "rb").read() == open(e["query"], "rb").read()
        for h in e["hits"]:
            assert os.path.isfile(h["path"]) and h["relevant"] is None and sum(h["concept_distances"]) == h["distance"]
    attn = np.load(os.path.join(out, "concept_attention.npy"))
    assert attn.shape == (3, 4, 14, 14) and attn.dtype == np.float32 and np.isfinite(attn).all() and (attn >= 0).all()
    total = attn.sum((2, 3))                    # the patch columns of softmax rows that also span the class and concept tokens
    assert (total > 0).all() and (total <= 1.0 + 1e-2).all()
