"""CPU: ranked lists of any depth, radius search and hash lookup -- the numpy restatement of tests/ranked_ref.py
against the C oracle's counting sort, retrieval.hash_lookup_stats (pure torch) against a brute force on the distance matrix, the argument
validation of ch_hamming_rank_scatter and of the Python entries (it runs before anything touches a GPU), and the configuration."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ranked_ref as rr
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbit,Qn,G", [(64, 9, 140), (128, 5, 131), (192, 3, 150)])
def test_restatement_equals_the_oracles_counting_sort(nbit, Qn, G):
    from oracle import hamming_oracle as ho
    labels = np.random.default_rng(1).integers(0, 3, G)
    centres = np.random.default_rng(2).integers(0, 2, (3, nbit)).astype(np.uint8)
    g = rr.clustered(labels, centres, nbit, 3)                  # deep buckets: every k cuts a tie
    q = rr.clustered(np.arange(Qn) % 3, centres, nbit, 4)
    g[-2:] = q[0]                                               # exact duplicates of a query at the very end of the gallery
    for k in (1, 129, G, G + 3):
        idx, dist = rr.ranked(q, g, k)
        ridx, rdist = ho.topk(q, g, k)
        assert np.array_equal(idx, ridx.astype(np.int64)) and np.array_equal(dist, rdist), k
    assert (idx[:, G:] == -1).all() and (dist[:, G:] == -1).all()
    assert idx[0, 0] == G - 2 and idx[0, 1] == G - 1 and dist[0, 1] == 0
    # radius, CSR and the fill are slices of the same ranking
    order, ds, d = rr.ranking(q, g)
    r = int(np.median(d))
    idx, dist = rr.ranked(q, g, 50, g_index_base=1000, radius=r)
    off, cidx, cdist = rr.radius_csr(q, g, r, g_index_base=1000, max_hits=50)
    for i in range(Qn):
        n = min(50, int((d[i] <= r).sum()))
        assert off[i + 1] - off[i] == n and np.array_equal(cidx[off[i]:off[i + 1]], idx[i, :n]) and (idx[i, n:] == -1).all()
        assert np.array_equal(cidx[off[i]:off[i + 1]] - 1000, order[i, :n]) and np.array_equal(cdist[off[i]:off[i + 1]], ds[i, :n])
    off, cidx, _ = rr.radius_csr(q, g, 64 * q.shape[1])
    assert np.array_equal(off, np.arange(Qn + 1) * G) and np.array_equal(cidx.reshape(Qn, G), order)


# ---- hash lookup -----------------------------------------------------------------------------------------------------------------
def _lookup_case(multi, seed):
    """30 x 400 clustered 64-bit codes; query 0 has no relevant row, query 1 is far from everything (small radii retrieve nothing)"""
    nbit, C = 64, 5
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 2, (C, nbit)).astype(np.uint8)
    gl = rng.integers(0, C - 1, 400)                              # class C - 1 never occurs in the gallery
    ql = rng.integers(0, C - 1, 30)
    ql[0] = C - 1
    g = rr.clustered(gl, centres, nbit, seed + 1)
    q = rr.clustered(ql, centres, nbit, seed + 2)
    q[1] = ~g[0]                                                  # 64 bits from g[0]: nothing within a small radius
    g[5] = q[2]                                                   # a distance-0 row
    if multi:
        qoh, goh = np.eye(C, dtype=np.uint8)[ql], np.eye(C, dtype=np.uint8)[gl]
        goh[rng.random(400) < 0.3, 0] = 1                         # multi-hot: some rows also carry class 0
        qoh[3, 1] = 1
        ql, gl = qoh, goh
    return q, g, ql, gl


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("remove_first", [False, True])
def test_hash_lookup_stats_equal_brute_force(multi, remove_first):
    from concepthash_amd import retrieval as rt
    q, g, ql, gl = _lookup_case(multi, 7)
    _, _, d = rr.ranking(q, g)
    rel = rr.relevance(ql, gl)
    assert not rel[0].any()                                       # the query without a relevant row
    radii = [0, 2, 8, 20, 64]
    want = rr.hash_lookup(d, rel, radii, remove_first)
    assert (want["retrieved"][1, :3] == 0).all() and want["retrieved"][2, 0] >= (0 if remove_first else 1)
    counts2 = rr.bucket_counts2(d, rel, 65)
    first = None
    if remove_first:
        top = np.argsort(d, axis=1, kind="stable")[:, 0]
        d0 = d[np.arange(len(q)), top]
        first = (torch.from_numpy(d0.astype(np.int64)), torch.from_numpy(rel[np.arange(len(q)), top].astype(np.int32)))
        assert np.array_equal(rt.lowest_bucket(torch.from_numpy(counts2)).numpy(), d0)
    for c2 in (torch.from_numpy(counts2), torch.from_numpy(counts2.astype(np.int32))):      # int32 is what the histogram pass leaves
        got = rt.hash_lookup_stats(c2, radii, first)
        assert np.array_equal(got["lookup_retrieved"].numpy(), want["retrieved"])
        assert np.array_equal(got["lookup_hits"].numpy(), want["hits"])
        for key, ref in (("precisions_radius", "precisions"), ("recalls_radius", "recalls"), ("retrieved_radius", "retrieved_mean"),
                         ("empty_radius", "empty")):
            assert np.abs(np.asarray(got[key]) - want[ref]).max() <= 1e-12, key
    assert got["empty_radius"][0] > 0 and got["empty_radius"][-1] == 0.0
    with pytest.raises(ValueError, match="radii"):
        rt.hash_lookup_stats(c2, [65])
    none = rt.hash_lookup_stats(torch.zeros(0, 65, 2, dtype=torch.int32), [0, 2])
    assert none["precisions_radius"] == [0.0, 0.0] and none["lookup_hits"].shape == (0, 2)


# ---- the entry's host-side checks ----------------------------------------------------------------------------------------------
def _scatter(lib, Qn=4, G=4, W=1, seg=256, q=1, g=1, base=1, start=1, limit=1, idx=1, dist=1):
    """the entry with dummy non-null pointers where a test needs one (every case below is refused before a pointer is read)"""
    return lib.ch_hamming_rank_scatter(q, Qn, g, G, W, seg, base, start, limit, 0, idx, dist, None)


def test_rank_scatter_refuses_bad_arguments_on_the_host(lib):
    from concepthash_amd import _lib
    assert "ch_hamming_rank_scatter" in _lib.SIGNATURES and lib.ch_abi_version() == 3
    for W in (0, 5, -1):
        assert _scatter(lib, W=W) == 2 and b"W" in lib.ch_last_error()
    for seg in (0, 65536, -3):
        assert _scatter(lib, seg=seg) == 2 and b"seg_rows" in lib.ch_last_error()
    assert _scatter(lib, Qn=-1) == 2 and b"negative" in lib.ch_last_error()
    assert _scatter(lib, G=-1) == 2 and b"negative" in lib.ch_last_error()
    for name in ("q", "g", "base", "start", "limit", "idx", "dist"):
        assert _scatter(lib, **{name: None}) == 2 and b"null" in lib.ch_last_error(), name
    assert _scatter(lib, G=70000 * 65535, seg=1) == 2                       # more than 2^32 - 1 rows / 65,535 segments
    # nothing to do: no launch, no pointer read
    assert _scatter(lib, Qn=0, q=None, base=None) == 0 and _scatter(lib, G=0, g=None, idx=None) == 0


def test_python_entries_refuse_what_is_not_built():
    from concepthash_amd import retrieval as rt
    from concepthash_amd.distributed import ShardedRetrieval
    q, g = torch.zeros(3, 2, dtype=torch.int64), torch.zeros(5, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="per-query mask"):
        rt.hamming_ranked(q, g, 200, mask=torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="per-query mask"):
        rt.hamming_radius(q, g, 2, mask=torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="k must be"):
        rt.hamming_ranked(q, g, 0)
    for r in (-1, 129):
        with pytest.raises(ValueError, match="radius"):
            rt.hamming_radius(q, g, r)
        with pytest.raises(ValueError, match="radius"):
            rt.hamming_ranked(q, g, 10, radius=r)
    with pytest.raises(NotImplementedError, match="radii"):
        ShardedRetrieval.__new__(ShardedRetrieval).evaluate(q, None, radii=[0, 2])
    # the chunks of queries cover [0, Qn) in order and keep hist + base under the budget
    chunks = list(rt._query_chunks(40000, 2_000_000, 4, None))
    assert chunks[0][0] == 0 and chunks[-1][1] == 40000 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and len(chunks) > 1
    for c0, c1, seg in chunks:
        assert 2 * -(-2_000_000 // seg) * 257 * 8 * (c1 - c0) <= rt.RANK_BUDGET_BYTES and 1 <= seg <= 65535


# ---- configuration -----------------------------------------------------------------------------------------------------------------
def test_radius_and_lookup_radii_configuration(tmp_path):
    import yaml
    import main_v2
    from concepthash_amd import config as cfglib
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yaml").write_text(yaml.safe_dump({"seed": 7, "model": {"nbit": 64}, "batch_size": 32, "exp": "hashing"}))
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", ["logdir=" + str(run), "dataset=synthetic_cub200", "k=1000", "radius=3"],
                         cwd=str(tmp_path))
    assert cfg.k == 1000 and cfg.radius == 3 and "radius" in main_v2.SEARCH_KEYS and all(k in cfg for k in main_v2.SEARCH_KEYS)
    laid = main_v2._run_config(cfg, "search", main_v2.SEARCH_KEYS)
    assert laid.exp == "search" and laid.k == 1000 and laid.radius == 3 and laid.model.nbit == 64
    plain = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", ["logdir=" + str(run), "dataset=synthetic_cub200"], cwd=str(tmp_path))
    assert plain.radius is None and plain.k == 10
    val = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", ["logdir=" + str(run), "dataset=synthetic_cub200"], cwd=str(tmp_path))
    assert val.hash_lookup_radii is None and "hash_lookup_radii" in main_v2.LOOP_KEYS
    on = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", ["logdir=" + str(run), "dataset=synthetic_cub200", "hash_lookup_radii=[0,2]"],
                        cwd=str(tmp_path))
    laid = main_v2._run_config(on, "validation", main_v2.EVAL_KEYS)
    assert list(laid.hash_lookup_radii) == [0, 2] and laid.exp == "validation" and laid.model.nbit == 64


@pytest.mark.parametrize("tie,concept", [(False, False), (True, False), (False, True), (True, True)])
def test_hash_lookup_evaluation_records_the_radii_beside_each_call(tmp_path, monkeypatch, tie, concept):
    """experiments.hash_lookup_eval.HashLookupEvaluation around a stub evaluator and a stub metric (no GPU): every calculate_mAP call of
    the evaluator asks for the radii, the four lists land beside the call's own key, the tie bracket and the per-concept table keep
    working beside it, and the rebound names are restored."""
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.hash_lookup_eval import HashLookupEvaluation
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, tie_bracket=False, PRs=None, radii=None, **k):
        seen.append((tuple(db_codes.shape), bool(tie_bracket), radii))
        m = float(db_codes.sum() + test_codes.sum())
        utils.hashing.last_tie_bracket = {"mAP_low": m - 1, "mAP_high": m + 1} if tie_bracket else None
        utils.hashing.last_hash_lookup = {"radii": radii, "precisions_radius": [m + r for r in radii], "recalls_radius": [m - r for r in radii],
                                          "retrieved_radius": [float(r) for r in radii], "empty_radius": [0.5] * len(radii)} if radii else None
        return m, [m] * len(PRs), [-m] * len(PRs)
    monkeypatch.setattr(utils.hashing, "calculate_mAP", metric)
    monkeypatch.setattr(base, "calculate_mAP", metric)
    db, te = torch.arange(5 * 12, dtype=torch.float32).reshape(5, 12), -torch.arange(3 * 12, dtype=torch.float32).reshape(3, 12) / 7

    def evaluator_main(self):
        res = {}
        res["mAP"], res["recalls"], res["precisions"] = base.calculate_mAP(db, None, te, None, -1, PRs=[1, 5], threshold=0)
        res["mAP_bin"], _, _ = base.calculate_mAP(db * 2, None, te * 2, None, -1, PRs=[1, 5], threshold=0)
        self.results = res
        return res
    monkeypatch.setattr(base.RetrievalEvaluation, "main", evaluator_main)
    ev = HashLookupEvaluation.__new__(HashLookupEvaluation)
    ev.config = _wrap({"hash_lookup_radii": [0, 2], "concept_eval": concept, "compute_mAP": True, "exp": "validation", "tie_bracket": tie,
                       "sub_code_eval": False, "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    m = float(db.sum() + te.sum())
    assert res["mAP"] == m and res["precisions_radius"] == [m, m + 2] and res["recalls_radius"] == [m, m - 2]
    assert res["retrieved_radius"] == [0.0, 2.0] and res["empty_radius"] == [0.5, 0.5] and res["precisions_radius_bin"] == [2 * m, 2 * m + 2]
    assert res["hash_lookup_radii"] == [0, 2]
    # only the whole-code calls take the radii; the per-concept slices pass through as they were
    assert [s for s in seen if s[0] == (5, 12)] == [((5, 12), tie, [0, 2])] * 2 and all(s[2] is None for s in seen if s[0] != (5, 12))
    assert len(seen) == (8 if concept else 2)
    assert ("mAP_tie_low" in res) == tie and ("mAP_concept" in res) == concept
    assert json.load(open(tmp_path / "history.json")) == res
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    if not concept and not tie:             # a top-level call whose result the evaluator does not store under one key is an error, not a skip
        def loses_one(self):
            res = evaluator_main(self)
            del res["mAP_bin"]
            return res
        monkeypatch.setattr(base.RetrievalEvaluation, "main", loses_one)
        with pytest.raises(RuntimeError, match="expected one key"):
            ev.main()
        assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
        monkeypatch.setattr(base.RetrievalEvaluation, "main", evaluator_main)
    ev.config["hash_lookup_radii"] = None                       # the key off: the evaluators below alone
    assert "precisions_radius" not in ev.main()
