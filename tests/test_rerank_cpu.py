"""CPU: the two-stage search ("two-stage") without a GPU -- the numpy reference of tests/rerank_ref.py against
itself, every argument error of the new surfaces (raised before any library call: the tensors here are host tensors, which no kernel
wrapper accepts), the config keys on their way to the experiments, and the evaluator class around a stub metric."""
import json
import os

import numpy as np
import pytest
import torch

import dense_ref as dref
import rerank_ref as rr
from conftest import ROOT


def _grid(rng, rows, n):
    return (rng.integers(-64, 65, (rows, n)) / 16.0).astype(np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", dref.METRICS)
def test_the_reference_with_a_shortlist_of_the_whole_gallery_is_the_exhaustive_list(metric):
    rng = np.random.default_rng(1)
    xq, xg = _grid(rng, 5, 48), _grid(rng, 90, 48)
    xg[rng.integers(0, 90, 30)] = xg[rng.integers(0, 90, 30)]           # equal distances: the index breaks them
    D = dref.dist(xq, xg, metric)
    for m, k in ((90, 10), (200, 90), (4096, 128)):
        idx, d = rr.two_stage(xq, xg, metric, m, k, D=D)
        want = dref.topk(D, k)
        assert np.array_equal(idx, want[0]) and np.array_equal(dref.bits(d), dref.bits(want[1]))
    # a shorter shortlist: the same set as the Hamming list, in the dense order
    cand = rr.shortlist(xq, xg, 20)
    idx, d = rr.two_stage(xq, xg, metric, 20, 20, D=D)
    assert np.array_equal(np.sort(idx, 1), np.sort(cand, 1))
    key = dref.order_key(d) << np.uint64(32) | idx.astype(np.uint64)
    assert np.all(key[:, 1:] >= key[:, :-1])
    # a radius leaves ragged lists; empty slots and a row listed twice in a hand-made list
    ragged = rr.shortlist(xq, xg, 20, radius=18)
    assert (ragged == -1).any() and (ragged != -1).any()
    hand = np.array([[3, -1, 7, 3, -1]] * 5)
    idx, d = rr.rerank(D, hand, 4)
    assert all(sorted(r[:3].tolist()) == [3, 3, 7] and r[3] == -1 for r in idx) and np.all(np.isposinf(d[:, 3]))
    assert rr.agreement(dref.topk(D, 10)[0], rr.two_stage(xq, xg, metric, 90, 10, D=D)[0], 10) == 1.0


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    from concepthash_amd import _lib

    def load():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", load)


def test_dense_rerank_refuses_bad_arguments_before_any_library_call(no_library):
    from concepthash_amd import retrieval as rt
    q, g = torch.zeros(3, 16), torch.ones(9, 16)
    cand = torch.zeros(3, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="metric must be one of"):
        rt.dense_rerank(q, g, cand, "manhattan", 2)
    with pytest.raises(ValueError, match="k must be"):
        rt.dense_rerank(q, g, cand, "dot", 9)
    with pytest.raises(ValueError, match="k must be"):
        rt.dense_rerank(q, g, cand, "dot", 0)
    with pytest.raises(ValueError, match="shortlist must be"):
        rt.dense_rerank(q, g, torch.zeros(3, 4097, dtype=torch.int64), "dot", 1)
    with pytest.raises(ValueError, match="shortlist must be"):
        rt.dense_rerank(q, g, torch.zeros(3, 0, dtype=torch.int64), "dot", 1)
    with pytest.raises(ValueError, match="cand must be"):
        rt.dense_rerank(q, g, cand.to(torch.int32), "dot", 2)
    with pytest.raises(ValueError, match="cand must be"):
        rt.dense_rerank(q, g, cand[:2], "dot", 2)
    with pytest.raises(ValueError, match="dimensions"):
        rt.dense_rerank(q, torch.ones(9, 17), cand, "dot", 2)
    with pytest.raises(ValueError, match="dimensions"):
        rt.dense_rerank(torch.zeros(3, 257), torch.ones(9, 257), cand, "dot", 2)
    bad = g.clone()
    bad[1, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        rt.dense_rerank(q, bad, cand, "cosine", 2)
    over = cand.clone()
    over[2, 5] = 9                                                      # one past the gallery
    with pytest.raises(ValueError, match="outside the gallery"):
        rt.dense_rerank(q, g, over, "euclidean", 2)
    with pytest.raises(ValueError, match="outside the gallery"):
        rt.dense_rerank(q, g, over + 100, "euclidean", 2, g_index_base=100)
    with pytest.raises(ValueError, match="g_index_base"):
        rt.dense_rerank(q, g, cand, "euclidean", 2, g_index_base=-1)
    # legal arguments on host tensors reach the launch, which has no CPU form: negative ids pass the validation
    with pytest.raises((AssertionError, RuntimeError)):
        rt.dense_rerank(q, g, cand - 1, "euclidean", 2)


def test_rerank_topk_and_evaluate_reranked_refuse_bad_arguments_before_any_library_call(no_library):
    from concepthash_amd import retrieval as rt
    q, g = torch.zeros(3, 16), torch.ones(9, 16)
    for k, m in ((0, 5), (6, 5), (1, 0), (1, 4097)):
        with pytest.raises(ValueError, match="must be in"):
            rt.rerank_topk(q, g, "cosine", k, m)
    with pytest.raises(ValueError, match="metric must be one of"):
        rt.rerank_topk(q, g, "hamming", 1, 5)
    with pytest.raises(ValueError, match="dimensions"):
        rt.rerank_topk(q, torch.ones(9, 12), "dot", 1, 5)
    ql, gl = torch.arange(3), torch.arange(9) % 3
    assert rt.check_shortlist(4096, 4096) == (4096, 4096) and rt.RERANK_MAX == 4096
    for R, ks in ((6, [1]), (0, [1]), (-2, [1]), ([2, 6], [1]), (5, [6]), (-1, [1, 6])):
        with pytest.raises(ValueError, match=r"must lie in \[1, shortlist = 5\]"):
            rt.evaluate_reranked(q, g, ql, gl, "cosine", 5, R, ks)
    with pytest.raises(ValueError, match="k >= 1"):
        rt.evaluate_reranked(q, g, ql, gl, "cosine", 5, 5, [0])
    with pytest.raises(ValueError, match="shortlist must be"):
        rt.evaluate_reranked(q, g, ql, gl, "cosine", 5000, -1, [1])
    with pytest.raises(ValueError, match="metric must be one of"):
        rt.evaluate_reranked(q, g, ql, gl, "l1", 5, -1, [1])


def test_search_and_calculate_map_refuse_a_shortlist_they_cannot_serve(no_library):
    from concepthash_amd.search import GalleryIndex
    from utils import hashing
    gen = torch.Generator().manual_seed(5)
    index = GalleryIndex(torch.randint(-2 ** 62, 2 ** 62, (7, 2), generator=gen, dtype=torch.int64), 120, 3, real=torch.randn(7, 120, generator=gen))
    x = torch.zeros(2, 120)
    for rank in ("hamming", "asymmetric", "ternary"):
        with pytest.raises(ValueError, match="shortlist with rank"):
            index.search(x, 3, rank=rank, shortlist=10)
    with pytest.raises(ValueError, match="k must be"):
        index.search(x, 11, rank="cosine", shortlist=10)
    with pytest.raises(ValueError, match="shortlist must be"):
        index.search(x, 3, rank="cosine", shortlist=4097)
    with pytest.raises(ValueError, match="radius must be"):
        index.search(x, 3, rank="cosine", shortlist=10, radius=129)
    with pytest.raises(ValueError, match="concepts"):
        index.search(x, 3, rank="euclidean", shortlist=10, concepts=[0])
    with pytest.raises(ValueError, match="margin"):
        index.search(x, 3, rank="dot", shortlist=10, margin=0.5)
    with pytest.raises(ValueError, match="radius"):                     # as before: no radius without a shortlist
        index.search(x, 3, rank="dot", radius=2)
    with pytest.raises(ValueError, match="not built"):                  # as before: k <= 128 without a shortlist
        index.search(x, 129, rank="dot")
    bare = GalleryIndex(index.codes, 120, 3)
    with pytest.raises(ValueError, match=r"real plane.*rebuild"):
        bare.search(x, 3, rank="cosine", shortlist=10)
    db, te = torch.randn(6, 16), torch.randn(3, 16)
    for rank in ("hamming", "asymmetric", "ternary"):
        with pytest.raises(ValueError, match="shortlist with rank"):
            hashing.calculate_mAP(db, torch.arange(6) % 2, te, torch.arange(3) % 2, -1, rank=rank, shortlist=4, margin=0.1)
    with pytest.raises(ValueError, match="shortlist must be"):
        hashing.calculate_mAP(db, torch.arange(6) % 2, te, torch.arange(3) % 2, -1, rank="dot", shortlist=0)


def test_calculate_map_hands_a_shortlist_to_evaluate_reranked(monkeypatch):
    import utils.hashing as hashing
    seen = []

    def evaluate_reranked(q, g, ql, gl, metric, shortlist, **k):
        seen.append((tuple(q.shape), tuple(g.shape), metric, shortlist, k))
        return {"mAP": 0.5, "recalls": [0.1], "precisions": [0.2], "R": 4, "agreement": {1: 0.75}}
    monkeypatch.setattr(hashing, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hashing.rt, "evaluate_reranked", evaluate_reranked)
    db, te = torch.randn(6, 16), torch.randn(3, 16)
    out = hashing.calculate_mAP(db, torch.arange(6) % 2, te, torch.arange(3) % 2, -1, PRs=[1], rank="dot", shortlist=4, remove_first_retrieved=True)
    assert out == (0.5, [0.1], [0.2])
    assert seen == [((3, 16), (6, 16), "dot", 4, dict(R=-1, ks=[1], remove_first=True, skip_queries_without_relevant=False))]
    assert hashing.last_rerank == dict(metric="dot", shortlist=4, R=4, agreement={1: 0.75})
    monkeypatch.setattr(hashing.rt, "evaluate_dense", lambda *a, **k: {"mAP": 0.25, "recalls": [], "precisions": []})
    assert hashing.calculate_mAP(db, torch.arange(6) % 2, te, torch.arange(3) % 2, -1, rank="dot")[0] == 0.25
    assert hashing.last_rerank is None                                  # ... after any other call


# ---- config keys -------------------------------------------------------------------------------------------------------------------
def test_the_shortlist_and_rerank_keys_reach_the_experiments(tmp_path):
    import yaml
    import main_v2
    from concepthash_amd import config as cfglib
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yaml").write_text(yaml.safe_dump({"seed": 7, "model": {"nbit": 64}, "batch_size": 32, "exp": "hashing"}))
    base = ["logdir=" + str(run), "dataset=synthetic_cub200"]
    cfgs = os.path.join(ROOT, "configs")
    val = cfglib.compose(cfgs, "val.yaml", base, cwd=str(tmp_path))
    assert val.rerank_eval is False and val.rerank_metric is None and val.rerank_shortlist is None
    assert all(k in main_v2.LOOP_KEYS for k in ("rerank_eval", "rerank_metric", "rerank_shortlist")) and "shortlist" in main_v2.SEARCH_KEYS
    on = cfglib.compose(cfgs, "val.yaml", base + ["rerank_eval=true", "rerank_metric=cosine", "rerank_shortlist=500"], cwd=str(tmp_path))
    laid = main_v2._run_config(on, "validation", main_v2.EVAL_KEYS)
    assert laid.rerank_eval is True and laid.rerank_metric == "cosine" and laid.rerank_shortlist == 500 and laid.exp == "validation"
    search = cfglib.compose(cfgs, "search.yaml", base, cwd=str(tmp_path))
    assert search.shortlist is None and all(k in search for k in main_v2.SEARCH_KEYS)
    search = cfglib.compose(cfgs, "search.yaml", base + ["rank=cosine", "shortlist=1000", "k=300", "radius=20"], cwd=str(tmp_path))
    laid = main_v2._run_config(search, "search", main_v2.SEARCH_KEYS)
    assert laid.shortlist == 1000 and laid.k == 300 and laid.radius == 20 and laid.rank == "cosine" and laid.exp == "search"


def test_rerank_evaluation_records_its_keys_beside_each_call(tmp_path, monkeypatch):
    """experiments.rerank_eval.RerankEvaluation around a stub evaluator and a stub metric: every whole-code call is followed by the same
    call with rank=<metric>, shortlist=<m>; the triple, the effective R and the agreement land beside the call's own key; the dense
    evaluator it extends still repeats its own call; the rebound names are restored; the settings have no defaults."""
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.rerank_eval import RerankEvaluation, check_rerank_settings
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, PRs=None, rank="hamming", shortlist=None, **k):
        seen.append((tuple(db_codes.shape), rank, shortlist, R))
        m = float(db_codes.sum()) + (0.5 if shortlist is not None else 0.25 if rank != "hamming" else 0.0)
        utils.hashing.last_rerank = dict(metric=rank, shortlist=shortlist, R=shortlist, agreement={1: 0.5, 5: m}) if shortlist is not None else None
        return m, [m] * len(PRs), [-m] * len(PRs)
    monkeypatch.setattr(utils.hashing, "calculate_mAP", metric)
    monkeypatch.setattr(base, "calculate_mAP", metric)
    db, te = torch.arange(5 * 12, dtype=torch.float32).reshape(5, 12) - 20, torch.zeros(3, 12)

    def evaluator_main(self):
        res = {}
        res["mAP"], res["recalls"], res["precisions"] = base.calculate_mAP(db, None, te, None, -1, PRs=[1, 5], threshold=0)
        res["mAP_bin"], _, _ = base.calculate_mAP(db * 2, None, te * 2, None, -1, PRs=[1, 5], threshold=0)
        self.results = res
        return res
    monkeypatch.setattr(base.RetrievalEvaluation, "main", evaluator_main)
    ev = RerankEvaluation.__new__(RerankEvaluation)
    ev.config = _wrap({"rerank_eval": True, "rerank_metric": "euclidean", "rerank_shortlist": 40, "dense_eval": True, "dense_metric": "dot",
                       "ternary_eval": False, "asymmetric_eval": False, "weight_bits": 8, "hash_lookup_radii": None, "concept_eval": False,
                       "compute_mAP": True, "exp": "validation", "tie_bracket": False, "sub_code_eval": False, "text_eval": False,
                       "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    m = float(db.sum())
    assert res["mAP"] == m and res["mAP_rerank"] == m + 0.5 and res["mAP_rerank_bin"] == 2 * m + 0.5 and res["mAP_dense"] == m + 0.25
    assert res["recalls_rerank"] == [m + 0.5] * 2 and res["precisions_rerank"] == [-m - 0.5] * 2
    assert res["rerank_metric"] == "euclidean" and res["rerank_shortlist"] == 40 and res["rerank_R"] == 40 and res["rerank_R_bin"] == 40
    assert res["rerank_agreement"] == {"1": 0.5, "5": m + 0.5} and res["rerank_agreement_bin"] == {"1": 0.5, "5": 2 * m + 0.5}
    assert seen == [((5, 12), "hamming", None, -1), ((5, 12), "euclidean", 40, -1), ((5, 12), "dot", None, -1)] * 2
    assert json.load(open(tmp_path / "history.json")) == res
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    ev.config["rerank_eval"] = False
    off = ev.main()
    assert "mAP_rerank" not in off and "rerank_metric" not in off and "mAP_dense" in off
    ev.config["rerank_eval"] = True
    for key, value, match in (("rerank_metric", None, "rerank_metric"), ("rerank_metric", "hamming", "rerank_metric"),
                              ("rerank_shortlist", None, "rerank_shortlist"), ("rerank_shortlist", 5000, "shortlist must be")):
        keep = ev.config[key]
        ev.config[key] = value
        with pytest.raises(ValueError, match=match):
            ev.main()
        ev.config[key] = keep
    assert check_rerank_settings("cosine", 4096) == ("cosine", 4096)
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric


def test_the_sharded_form_is_refused(monkeypatch):
    from concepthash_amd.distributed import RowShard
    from utils import hashing
    shard = RowShard.__new__(RowShard)
    with pytest.raises(NotImplementedError, match="sharded"):
        hashing.calculate_mAP(shard, shard, torch.zeros(2, 16), torch.zeros(2), -1, rank="cosine", shortlist=10)
