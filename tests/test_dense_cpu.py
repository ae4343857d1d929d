"""CPU: the rankings of real-valued codes (csrc/dense_rank.hip) -- the fp64 reference of tests/dense_ref.py
against the Hamming order on sign codes, the host-side checks of the C entries, the argument rules of `calculate_mAP`,
`calculate_pr_curve` and `GalleryIndex.search` under rank="cosine" | "euclidean" | "dot" with the GPU taken away, the index file with
and without its real plane, the evaluator's keys and the two config keys.  No kernel runs here."""
import json
import os
import re

import numpy as np
import pytest
import torch

import dense_ref as dref
from conftest import ROOT

NEW_SYMBOLS = ("ch_dense_prepared_bytes", "ch_dense_prepare", "ch_dense_dist", "ch_dense_topk_seg_rows", "ch_dense_topk_workspace",
               "ch_dense_topk", "ch_dense_rank_collect", "ch_dense_rank_count")


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", dref.METRICS)
def test_the_reference_reproduces_the_hamming_order_on_sign_codes(metric):
    rng = np.random.default_rng(1)
    n = 64
    q, g = np.where(rng.random((9, n)) < 0.5, -1.0, 1.0), np.where(rng.random((300, n)) < 0.5, -1.0, 1.0)
    h = dref.hamming(q, g)
    D = dref.dist(q, g, metric)
    want = {"dot": 2.0 * h - n, "euclidean": 4.0 * h, "cosine": 2.0 * h / n}[metric]
    assert np.array_equal(D, want)
    index = np.arange(300)
    for i in range(9):
        assert np.array_equal(np.lexsort((index, D[i])), np.lexsort((index, h[i])))
    assert np.array_equal(dref.topk(D, 10)[0], dref.topk(h.astype(np.float64), 10)[0])


def test_the_reference_order_key_bounds_and_bracket():
    d = np.array([-np.inf, -3e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.5, 3e38, np.inf], np.float32)
    o = dref.order_key(d)
    assert np.all(o[1:] >= o[:-1]) and o[4] == o[5] == 0x80000000 and np.all(np.diff(o.astype(np.int64))[[0, 1, 2, 3, 5, 6, 7, 8]] > 0)
    rng = np.random.default_rng(2)
    q, g = rng.standard_normal((5, 48)).astype(np.float32), rng.standard_normal((40, 48)).astype(np.float32)
    q[1] = 0.0
    assert np.all(dref.dist(q, g, "cosine")[1] == 1.0)                  # a zero row: distance 1 to everything
    for metric in dref.METRICS:                                         # fp32 chains in the kernels' order stay inside the bounds
        D, E = dref.dist(q, g, metric), dref.bound(q, g, metric)
        qq, gg = (q, g) if metric != "cosine" else (dref.normalise(q).astype(np.float32), dref.normalise(g).astype(np.float32))
        acc = np.zeros((5, 40), np.float32)
        for j in range(48):                                             # products rounded before the sum: a looser chain than fmaf
            t = (qq[:, None, j] - gg[None, :, j]) if metric == "euclidean" else None
            acc = (acc + (t * t if metric == "euclidean" else qq[:, None, j] * gg[None, :, j])).astype(np.float32)
        got = {"dot": -acc, "euclidean": acc, "cosine": np.float32(1.0) - acc}[metric]
        assert np.all(np.abs(got - D) <= 2 * E + 1e-30), metric
    # the bracket: two rows closer than their bounds may swap, a third far away may not
    D = np.array([[0.10, 0.10 + 1e-9, 0.5]])
    E = np.full((1, 3), 1e-8)
    lo, hi = dref.ap_bracket(D, E, np.array([[False, True, True]]))
    assert hi[0] == pytest.approx((1 / 1 + 2 / 3) / 2) and lo[0] == pytest.approx((1 / 2 + 2 / 3) / 2)
    lo, hi = dref.ap_bracket(D, np.zeros((1, 3)), np.array([[False, True, True]]))
    assert lo[0] == hi[0] == pytest.approx((1 / 2 + 2 / 3) / 2)
    # merging two shards' lists by (ord(D), index)
    Dm = rng.standard_normal((4, 30)).astype(np.float32).astype(np.float64)
    a, b = dref.topk(Dm[:, :12], 7), dref.topk(Dm[:, 12:], 7, base=12)
    merged = dref.merge_lists([a[0], b[0]], [a[1], b[1]], 7)
    assert np.array_equal(merged[0], dref.topk(Dm, 7)[0]) and np.array_equal(merged[1], dref.topk(Dm, 7)[1])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    from concepthash_amd import _lib
    header = open(os.path.join(ROOT, "include", "concepthash_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\s*\(", code), name
    assert int(re.search(r"#define CH_ABI_VERSION (\d+)", header).group(1)) == 3 == _lib.ABI_VERSION
    from concepthash_amd import build
    assert "dense_rank.hip" in build.SOURCES and build.EXTRA_FLAGS["dense_rank.hip"] == ["-ffp-contract=off"]


def test_the_entries_check_their_arguments_on_the_host():
    from concepthash_amd import _lib, build
    build.build()
    lib = _lib.load()
    err = lambda: lib.ch_last_error().decode()
    assert lib.ch_dense_prepared_bytes(131, 48) == 192 * 48 * 4 and lib.ch_dense_prepared_bytes(64, 1) == 256
    assert lib.ch_dense_prepared_bytes(0, 48) == 0
    for n in (0, 257):
        assert lib.ch_dense_prepare(None, 4, n, 0, None, None) == 2 and "dense_prepare" in err() and "n must be" in err()
        assert lib.ch_dense_dist(None, 4, None, 4, n, 0, None, None) == 2 and "dense_dist" in err()
        assert lib.ch_dense_topk(None, 4, None, 4, n, 0, 10, 0, 0, None, None, None, 0, None) == 2 and "dense_topk" in err()
        assert lib.ch_dense_rank_collect(None, 4, None, 4, n, 0, None, None, 0, 0, None, None, None, None) == 2 and "dense_rank_collect" in err()
        assert lib.ch_dense_rank_count(None, 4, None, 4, n, 0, 0, 256, None, None, 16, None, None) == 2 and "dense_rank_count" in err()
    for metric in (-1, 3):
        assert lib.ch_dense_prepare(None, 4, 16, metric, None, None) == 2 and "metric" in err()
        assert lib.ch_dense_topk(None, 4, None, 4, 16, metric, 10, 0, 0, None, None, None, 0, None) == 2 and "metric" in err()
    assert lib.ch_dense_prepare(None, 4, 16, 0, None, None) == 2 and "null pointer" in err()
    assert lib.ch_dense_prepare(None, 0, 16, 0, None, None) == 0 and lib.ch_dense_prepare(None, -1, 16, 0, None, None) == 2
    assert lib.ch_dense_dist(None, 4, None, 4, 16, 1, None, None) == 2 and "null pointer" in err()
    assert lib.ch_dense_dist(None, 0, None, 4, 16, 1, None, None) == 0 and lib.ch_dense_dist(None, 4, None, 0, 16, 1, None, None) == 0
    for k in (0, 129):
        assert lib.ch_dense_topk(None, 4, None, 4, 16, 2, k, 0, 0, None, None, None, 0, None) == 2 and "k <= 128" in err()
    assert lib.ch_dense_topk(None, 4, None, 4, 16, 2, 10, (1 << 32) - 3, 0, None, None, None, 0, None) == 2 and "g_index_base" in err()
    assert lib.ch_dense_topk(None, 4, None, 4, 16, 2, 10, -1, 0, None, None, None, 0, None) == 2 and "g_index_base" in err()
    assert lib.ch_dense_topk(None, 4, None, 4, 16, 2, 10, 0, -1, None, None, None, 0, None) == 2 and "seg_rows" in err()
    assert lib.ch_dense_topk(None, 4, None, 4, 16, 2, 10, 0, 0, None, None, None, 0, None) == 2 and "null pointer" in err()
    assert lib.ch_dense_topk(None, 0, None, 4, 16, 2, 10, 0, 0, None, None, None, 0, None) == 0
    assert lib.ch_dense_rank_collect(None, 4, None, 4, 16, 0, None, None, 0, (1 << 32) - 3, None, None, None, None) == 2 and "g_index_base" in err()
    assert lib.ch_dense_rank_collect(None, 4, None, 4, 16, 0, None, None, -1, 0, None, None, None, None) == 2 and "LW" in err()
    assert lib.ch_dense_rank_collect(None, 0, None, 4, 16, 0, None, None, 0, 0, None, None, None, None) == 0
    assert lib.ch_dense_rank_count(None, 4, None, 4, 16, 0, 0, 0, None, None, 16, None, None) == 2 and "seg_rows" in err()
    for cap in (0, 8193):
        assert lib.ch_dense_rank_count(None, 4, None, 4, 16, 0, 0, 256, None, None, cap, None, None) == 2 and "list_cap" in err()
    assert lib.ch_dense_rank_count(None, 4, None, 1 << 30, 16, 0, 0, 1, None, None, 16, None, None) == 2 and "null pointer" in err()
    # the segmentation of the scan's own choice: whole trips of 256 rows, at most 65,535 segments, the workspace that goes with it
    for Qn, G in [(1, 1), (70, 771), (1024, 1_000_000), (5794, 5994), (3, 40_000_000), (100_000, 5000)]:
        seg = lib.ch_dense_topk_seg_rows(Qn, G)
        nseg = -(-G // seg)
        assert seg % 256 == 0 and 1 <= nseg <= 65535, (Qn, G, seg)
        assert lib.ch_dense_topk_workspace(Qn, G, 10, 0) == nseg * Qn * 10 * 8 + 16
        assert lib.ch_dense_topk_workspace(Qn, G, 10, 256) == -(-G // 256) * Qn * 10 * 8 + 16


# ---- retrieval.py without a GPU --------------------------------------------------------------------------------------------------
def test_python_entries_check_their_arguments_without_a_gpu():
    from concepthash_amd import retrieval as rt
    assert rt.DENSE_METRICS == ("cosine", "euclidean", "dot")
    with pytest.raises(ValueError, match="metric must be one of"):
        rt.prepare_dense(torch.zeros(3, 8), "manhattan")
    with pytest.raises(ValueError, match="2-D"):
        rt.prepare_dense(torch.zeros(8), "dot")
    for n in (0, 257):
        with pytest.raises(ValueError, match="dimensions"):
            rt.prepare_dense(torch.zeros(3, n), "dot")
    for bad in (float("nan"), float("inf"), -float("inf")):
        x = torch.zeros(3, 8)
        x[1, 5] = bad
        with pytest.raises(ValueError, match="finite"):
            rt.prepare_dense(x, "cosine")
        with pytest.raises(ValueError, match="finite"):
            rt.evaluate_dense(torch.zeros(2, 8), x, torch.zeros(2), torch.zeros(3), "dot")
    q, g = rt.DenseCodes(torch.zeros(64 * 8), 3, 8, "dot"), rt.DenseCodes(torch.zeros(64 * 8), 5, 8, "cosine")
    with pytest.raises(ValueError, match="prepared for"):
        rt.dense_dist(q, g)
    with pytest.raises(ValueError, match="prepared for"):
        rt.dense_topk(q, q, "cosine", 3)
    with pytest.raises(TypeError):
        rt.dense_topk(torch.zeros(3, 8), q, "dot", 3)
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must be"):
            rt.dense_topk(q, q, "dot", k)
    with pytest.raises(ValueError, match="dimensions"):
        rt.dense_dist(q, rt.DenseCodes(torch.zeros(64 * 9), 5, 9, "dot"))
    with pytest.raises(ValueError, match="k >= 1"):
        rt.evaluate_dense(torch.zeros(2, 8), torch.zeros(3, 8), torch.zeros(2), torch.zeros(3), "dot", ks=(0,))
    with pytest.raises(ValueError, match="dimensions"):
        rt.evaluate_dense(torch.zeros(2, 8), torch.zeros(3, 9), torch.zeros(2), torch.zeros(3), "dot")
    out = rt.evaluate_dense(torch.zeros(0, 8), torch.zeros(3, 8), torch.zeros(0), torch.zeros(3), "cosine", R=[5, -1])
    assert out["mAP"] == [0.0, 0.0] and out["hits"].shape == (0, 3) and len(out["S"]) == 2
    out = rt.evaluate_dense(torch.zeros(2, 8), torch.zeros(0, 8), torch.zeros(2), torch.zeros(0), "euclidean")
    assert set(out) == {"mAP", "precisions", "recalls", "hits", "total", "S", "nrel", "ap"} and out["S"].shape == (2,)
    # the order key and the unsigned sort are plain torch
    d = torch.tensor([-1.5, -0.0, 0.0, 2.0 ** -140, 1.5, float("inf")])
    o = rt.dense_order(d)
    assert np.array_equal(o.numpy().astype(np.uint64), dref.order_key(d.numpy())) and o[1] == o[2] == 0x80000000
    assert torch.equal(rt.dense_unorder(o).view(torch.int32), (d + 0.0).view(torch.int32))
    keys = torch.tensor([-1, 0, 1 << 62, -(1 << 63), 5, -7, 3], dtype=torch.int64)      # uint64 bit patterns
    offsets = torch.tensor([0, 4, 4, 7])
    got = rt.sort_slices_unsigned(offsets, keys).numpy().view(np.uint64)
    want = np.concatenate([np.sort(keys.numpy().view(np.uint64)[a:b]) for a, b in ((0, 4), (4, 4), (4, 7))])
    assert np.array_equal(got, want) and got[3] == 2 ** 64 - 1


def test_the_one_slice_sort_against_numpy_on_each_of_its_paths():
    """`sort_slices` (and `sort_slices_unsigned`, its `wide` form) against np.sort per slice: keys below 2^48 with few slices (the
    single sort of slice << 48 | key), keys that use all 64 bits, and more than 32,767 slices of keys below 2^48 (the flipped-top-bit
    two-sort, told to expect small keys)."""
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(11)

    def case(lengths, keys_u64, sort):
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        assert offsets[-1] == keys_u64.size
        got = sort(torch.from_numpy(offsets), torch.from_numpy(keys_u64.view(np.int64).copy())).numpy().view(np.uint64)
        want = np.concatenate([np.sort(keys_u64[a:b]) for a, b in zip(offsets[:-1], offsets[1:])])
        assert np.array_equal(got, want)

    few = rng.integers(0, 40, 300)
    few[[0, 7, 299]] = 0                                                   # empty slices, the first and the last among them
    small = rng.integers(0, 1 << 48, int(few.sum()), dtype=np.uint64)
    small[:5] = [0, (1 << 48) - 1, 65279 << 32, (1 << 32) - 1, 1 << 47]    # the ends of the range, of the distance and of the index
    case(few, small, rt.sort_slices)
    case(few, small, rt.sort_slices_unsigned)                              # the flip is harmless for small keys
    wide = rng.integers(0, 1 << 64, int(few.sum()), dtype=np.uint64, endpoint=False)
    wide[:4] = [0, 2 ** 64 - 1, 1 << 63, (1 << 63) - 1]
    case(few, wide, rt.sort_slices_unsigned)
    case(few, wide, lambda o, k: rt.sort_slices(o, k, wide=True))
    many = rng.integers(0, 3, 0x7FFF + 2)                                  # 32,769 slices: their number does not fit above a key
    small = rng.integers(0, 1 << 48, int(many.sum()), dtype=np.uint64)
    small[:2] = [(1 << 48) - 1, 0]
    case(many, small, rt.sort_slices)


# ---- calculate_mAP / calculate_pr_curve ------------------------------------------------------------------------------------------
def test_calculate_map_refuses_before_it_touches_a_gpu(monkeypatch):
    import utils.hashing as hashing

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(hashing, "_device", no_gpu)
    monkeypatch.setattr(hashing.rt, "pack_sign", no_gpu)
    monkeypatch.setattr(hashing.rt, "prepare_dense", no_gpu)
    monkeypatch.setattr(hashing.rt, "evaluate_dense", no_gpu)
    assert hashing.RANKS == ("hamming", "asymmetric", "ternary", "cosine", "euclidean", "dot")
    db, te = torch.randn(6, 16), torch.randn(3, 16)
    dl, tl = torch.arange(6) % 2, torch.arange(3) % 2
    with pytest.raises(ValueError, match="rank must be one of"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="manhattan")
    for rank in ("cosine", "euclidean", "dot"):
        with pytest.raises(ValueError, match="tie bracket"):
            hashing.calculate_mAP(db, dl, te, tl, -1, rank=rank, tie_bracket=True)
        with pytest.raises(ValueError, match="radius"):
            hashing.calculate_mAP(db, dl, te, tl, -1, rank=rank, radii=[0, 2])
        from concepthash_amd.distributed import RowShard
        shard = RowShard.__new__(RowShard)
        with pytest.raises(NotImplementedError, match="sharded"):
            hashing.calculate_mAP(shard, shard, te, tl, -1, rank=rank)
        with pytest.raises(NotImplementedError, match="sharded"):
            hashing.calculate_pr_curve(shard, shard, te, tl, rank=rank)
        for bad in (float("nan"), float("inf")):
            x = db.clone()
            x[2, 3] = bad
            with pytest.raises(ValueError, match="finite"):
                hashing.calculate_mAP(x, dl, te, tl, -1, rank=rank)
            with pytest.raises(ValueError, match="finite"):
                hashing.calculate_mAP(db, dl, x[:3], tl, -1, rank=rank)
        with pytest.raises(ValueError, match="dimensions"):
            hashing.calculate_mAP(torch.randn(6, 300), dl, torch.randn(3, 300), tl, -1, rank=rank)
        # dist_metric is what it was: it raises, and now says which argument asks for these rankings
        with pytest.raises(NotImplementedError, match=r'rank="cosine" \| "euclidean" \| "dot"'):
            hashing.calculate_mAP(db, dl, te, tl, -1, rank=rank, dist_metric=rank)
    with pytest.raises(NotImplementedError, match="rank="):
        hashing.calculate_mAP(db, dl, te, tl, -1, dist_metric="cosine")
    with pytest.raises(NotImplementedError, match="rank="):
        hashing.calculate_pr_curve(db, dl, te, tl, dist_metric="cosine")
    for rank in ("ternary", "asymmetric", "manhattan"):
        with pytest.raises(ValueError, match="rank must be"):
            hashing.calculate_pr_curve(db, dl, te, tl, rank=rank)


def test_calculate_map_hands_both_real_code_sets_to_the_dense_evaluation(monkeypatch):
    import utils.hashing as hashing
    seen = []

    def evaluate_dense(q, g, ql, gl, metric, **k):
        seen.append((tuple(q.shape), tuple(g.shape), q.dtype, metric, k))
        n = len(k["R"]) if isinstance(k["R"], list) else 0
        return {"mAP": [0.5] * n if n else 0.5, "recalls": [0.1], "precisions": [0.2], "total": torch.tensor([2, 0, 1]),
                "nrel": [torch.tensor([1, 0, 1])] * n}
    monkeypatch.setattr(hashing, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hashing.rt, "evaluate_dense", evaluate_dense)
    db, te = torch.randn(6, 16, dtype=torch.float64), torch.randn(3, 16)
    out = hashing.calculate_mAP(db, torch.arange(6) % 2, te, torch.arange(3) % 2, 50, PRs=[5], rank="euclidean", remove_first_retrieved=True,
                                skip_queries_without_relevant=True)
    assert out == (0.5, [0.1], [0.2])
    assert seen == [((3, 16), (6, 16), torch.float32, "euclidean", dict(R=50, ks=[5], remove_first=True, skip_queries_without_relevant=True))]
    assert hashing.last_tie_bracket is None and hashing.last_hash_lookup is None
    recalls, precisions, Rs = hashing.calculate_pr_curve(db, torch.arange(6) % 2, te, torch.arange(3) % 2, Rs=[2, 4], rank="cosine")
    assert Rs == [2, 4] and seen[1][3] == "cosine" and seen[1][4]["R"] == [2, 4] and seen[1][4]["ks"] == []
    assert precisions == pytest.approx([(1 / 2 + 0 + 1 / 2) / 3, (1 / 4 + 0 + 1 / 4) / 3]) and recalls == pytest.approx([(0.5 + 0 + 1) / 3] * 2)


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------
def test_val_yaml_composes_with_the_two_keys(tmp_path):
    import yaml
    import main_v2
    from concepthash_amd import config as cfglib
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yaml").write_text(yaml.safe_dump({"seed": 7, "model": {"nbit": 64}, "batch_size": 32, "exp": "hashing"}))
    base = ["logdir=" + str(run), "dataset=synthetic_cub200"]
    val = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", base, cwd=str(tmp_path))
    assert val.dense_eval is False and val.dense_metric is None
    assert "dense_eval" in main_v2.LOOP_KEYS and "dense_metric" in main_v2.LOOP_KEYS
    on = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", base + ["dense_eval=true", "dense_metric=cosine"], cwd=str(tmp_path))
    laid = main_v2._run_config(on, "validation", main_v2.EVAL_KEYS)
    assert laid.dense_eval is True and laid.dense_metric == "cosine" and laid.exp == "validation"
    search = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", base + ["rank=cosine"], cwd=str(tmp_path))
    assert search.rank == "cosine" and all(k in search for k in main_v2.SEARCH_KEYS)


@pytest.mark.parametrize("tie,concept,radii,ternary", [(False, False, None, False), (True, True, [0, 2], True)])
def test_dense_evaluation_records_its_keys_beside_each_call(tmp_path, monkeypatch, tie, concept, radii, ternary):
    """experiments.dense_eval.DenseEvaluation around a stub evaluator and a stub metric: every whole-code call is followed by the same
    call under the dense rank (without the bracket and the radii), the triple and the gap land beside the call's own key, the evaluators
    it extends -- the ternary one included -- still find what the Hamming call left behind, and the rebound names are restored."""
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.dense_eval import DenseEvaluation
    seen = []
    shift = {"hamming": 0.0, "asymmetric": 0.25, "ternary": 0.5, "dot": 0.75}

    def metric(db_codes, db_labels, test_codes, test_labels, R, tie_bracket=False, PRs=None, radii=None, rank="hamming", weight_bits=8,
               margin=None, **k):
        seen.append((tuple(db_codes.shape), bool(tie_bracket), radii, rank, margin))
        m = float(db_codes.sum() + test_codes.sum()) + shift[rank]
        utils.hashing.last_tie_bracket = {"mAP_low": m - 1, "mAP_high": m + 1} if tie_bracket else None
        utils.hashing.last_hash_lookup = {"radii": radii, "precisions_radius": [m + r for r in radii], "recalls_radius": [m - r for r in radii],
                                          "retrieved_radius": [float(r) for r in radii], "empty_radius": [0.5] * len(radii)} if radii else None
        return m, [m] * len(PRs), [-m] * len(PRs)
    monkeypatch.setattr(utils.hashing, "calculate_mAP", metric)
    monkeypatch.setattr(base, "calculate_mAP", metric)
    db, te = torch.arange(5 * 12, dtype=torch.float32).reshape(5, 12) - 20, -torch.arange(3 * 12, dtype=torch.float32).reshape(3, 12) / 7

    def evaluator_main(self):
        res = {}
        res["mAP"], res["recalls"], res["precisions"] = base.calculate_mAP(db, None, te, None, -1, PRs=[1, 5], threshold=0)
        res["mAP_bin"], _, _ = base.calculate_mAP(db * 2, None, te * 2, None, -1, PRs=[1, 5], threshold=0)
        self.results = res
        return res
    monkeypatch.setattr(base.RetrievalEvaluation, "main", evaluator_main)
    ev = DenseEvaluation.__new__(DenseEvaluation)
    ev.config = _wrap({"dense_eval": True, "dense_metric": "dot", "ternary_eval": ternary, "ternary_margin": 2.5, "asymmetric_eval": False,
                       "weight_bits": 8, "hash_lookup_radii": radii, "concept_eval": concept, "compute_mAP": True, "exp": "validation",
                       "tie_bracket": tie, "sub_code_eval": False, "text_eval": False, "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    m = float(db.sum() + te.sum())
    assert res["mAP"] == m and res["mAP_dense"] == m + 0.75 and res["mAP_dense_bin"] == 2 * m + 0.75 and res["dense_metric"] == "dot"
    assert res["recalls_dense"] == [m + 0.75] * 2 and res["precisions_dense"] == [-m - 0.75] * 2
    assert res["quantisation_gap"] == res["mAP_dense"] - res["mAP"] and res["quantisation_gap_bin"] == res["mAP_dense_bin"] - res["mAP_bin"]
    assert "recalls_dense_bin" in res and "precisions_dense_bin" in res
    whole = [s for s in seen if s[0] == (5, 12)]
    per_call = [((5, 12), tie, radii, "hamming", None), ((5, 12), False, None, "dot", None)] + \
        ([((5, 12), False, None, "ternary", 2.5)] if ternary else [])
    assert whole == per_call * 2
    assert all(s[3] == "hamming" for s in seen if s[0] != (5, 12)) and len(seen) == len(whole) + (6 if concept else 0)
    assert ("mAP_tie_low" in res) == tie and ("mAP_concept" in res) == concept and ("precisions_radius" in res) == (radii is not None)
    assert ("mAP_ternary" in res) == ternary
    if tie:
        assert res["mAP_tie_low"] == m - 1 and res["mAP_tie_high_bin"] == 2 * m + 1      # the Hamming call's bracket, not None
    if radii:
        assert res["precisions_radius"] == [m, m + 2]
    if ternary:
        assert res["mAP_ternary"] == m + 0.5 and res["mAP_ternary_bin"] == 2 * m + 0.5
    assert json.load(open(tmp_path / "history.json")) == res
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    ev.config["dense_eval"] = False                             # the key off: the evaluators below alone
    seen.clear()
    off = ev.main()
    assert "mAP_dense" not in off and "dense_metric" not in off and "quantisation_gap" not in off and all(s[3] != "dot" for s in seen)
    ev.config["dense_eval"], ev.config["dense_metric"] = True, None
    with pytest.raises(ValueError, match="dense_metric"):       # required: there is no default
        ev.main()
    ev.config["dense_metric"] = "manhattan"
    with pytest.raises(ValueError, match="dense_metric"):
        ev.main()
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric


# ---- the index -------------------------------------------------------------------------------------------------------------------
def _index(with_real, nbit=120, Q=3, G=7):
    from concepthash_amd.search import GalleryIndex
    g = torch.Generator().manual_seed(5)
    W = (nbit + 63) // 64
    codes = torch.randint(-2 ** 62, 2 ** 62, (G, W), generator=g, dtype=torch.int64)
    real = torch.randn(G, nbit, generator=g) if with_real else None
    return GalleryIndex(codes, nbit, Q, labels=torch.arange(G) % 3, transform={"resize": 256, "crop": 224, "norm": 2},
                        fingerprint={"file": "best.pth", "size": 11, "sha256": "ab" * 32}, real=real)


@pytest.mark.parametrize("with_real", [True, False])
def test_gallery_index_round_trip_with_and_without_the_real_plane(tmp_path, with_real):
    from concepthash_amd import search
    from concepthash_amd.search import GalleryIndex
    a = _index(with_real)
    path = str(tmp_path / "index.pth")
    a.save(path)
    raw = torch.load(path, map_location="cpu")
    old = {"format", "codes", "nbit", "ncontext", "labels", "paths", "data_root", "mean", "transform", "fingerprint"}
    assert raw["format"] == 1 == search.FORMAT and set(raw) == (old | {"real"} if with_real else old)
    b = GalleryIndex.load(path, fingerprint=dict(a.fingerprint), nbit=120)
    assert torch.equal(a.codes, b.codes) and b.mask is None and b.margin is None
    assert (b.real is None) == (not with_real) and (b.real is None or (torch.equal(a.real, b.real) and b.real.dtype == torch.float32))
    c = b.to("cpu")
    assert (c.real is None) == (not with_real)


def test_an_index_file_written_without_the_plane_still_loads_and_search_names_what_the_dense_ranks_need(tmp_path):
    from concepthash_amd import search
    from concepthash_amd.search import GalleryIndex
    a = _index(False)
    path = str(tmp_path / "index.pth")
    torch.save({"format": 1, "codes": a.codes, "nbit": a.nbit, "ncontext": a.ncontext, "labels": a.labels, "paths": None, "data_root": None,
                "mean": None, "transform": a.transform, "fingerprint": a.fingerprint}, path)         # the file of before, key for key
    b = GalleryIndex.load(path, fingerprint=dict(a.fingerprint), nbit=120)
    assert b.real is None and torch.equal(b.codes, a.codes)
    assert search.RANKS == ("hamming", "asymmetric", "ternary", "cosine", "euclidean", "dot")
    for rank in ("cosine", "euclidean", "dot"):
        with pytest.raises(ValueError, match=r"real plane.*rebuild"):
            b.search(torch.zeros(2, 120), 3, rank=rank)
    r = _index(True)
    with pytest.raises(ValueError, match="not built"):
        r.search(torch.zeros(2, 120), 129, rank="cosine")
    with pytest.raises(ValueError, match="not built"):
        r.search(torch.zeros(2, 120), 0, rank="cosine")
    with pytest.raises(ValueError, match="concepts"):
        r.search(torch.zeros(2, 120), 3, rank="euclidean", concepts=[0])
    with pytest.raises(ValueError, match="margin"):
        r.search(torch.zeros(2, 120), 3, rank="dot", margin=0.1)
    with pytest.raises(ValueError, match="radius"):
        r.search(torch.zeros(2, 120), 3, rank="dot", radius=2)
    with pytest.raises(ValueError, match="query codes must be"):
        r.search(torch.zeros(2, 64), 3, rank="dot")
    x = torch.zeros(2, 120)
    x[0, 0] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        r.search(x, 3, rank="cosine")
    with pytest.raises(ValueError, match="rank must be one of"):
        r.search(torch.zeros(2, 120), 3, rank="manhattan")
    with pytest.raises(ValueError, match="real"):
        GalleryIndex(a.codes, 120, 3, real=torch.zeros(3, 120))
    bad = torch.zeros(7, 120)
    bad[3, 3] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        GalleryIndex(a.codes, 120, 3, real=bad)
