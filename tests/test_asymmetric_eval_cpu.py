"""No GPU: the rank-count identity behind the evaluation of the weighted (asymmetric) ranking (DESIGN.md section 2.0,
csrc/hamming_rankcount.hip) against the brute-force reference of tests/asymmetric_eval_ref.py, and the surface around it -- the header
and the binding name the three entries, `calculate_mAP` refuses what the ranking does not define before it touches a GPU, the
evaluator's keys compose, and `AsymmetricEvaluation` records the asymmetric triple beside every whole-code call."""
import json
import os
import re

import numpy as np
import pytest
import torch

import asymmetric_eval_ref as aref
import weighted_topk_ref as wref
from conftest import ROOT

ENTRIES = ("ch_hamming_rank_collect", "ch_hamming_rank_count", "ch_hamming_rank_ap")


def _problem(rng, t):
    """one tiny problem: (D, rel, limits, remove_first, base)"""
    nbit = (16, 48, 64, 128)[t % 4]
    bits = (4, 8)[(t // 4) % 2]
    G = int(rng.integers(1, 200))
    Qn = int(rng.integers(1, 6))
    C = int(rng.integers(1, 6))
    g_codes = rng.standard_normal((G, nbit)).astype(np.float32)
    if G > 3:                                                       # duplicate gallery rows: equal D is common
        src = rng.integers(0, G, G // 2)
        g_codes[rng.integers(0, G, G // 2)] = g_codes[src]
    codes = rng.standard_normal((Qn, nbit)).astype(np.float32)
    if t % 5 == 0:
        codes[0] = 0.0                                              # an all-zero query: every D is 0, the ranking is by index
    g = wref.pack_sign(g_codes)
    D = aref.distances(codes, g, bits)
    if t % 3 == 0:                                                  # multi-hot
        ql = (rng.random((Qn, C)) < 0.4).astype(np.int64)
        gl = (rng.random((G, C)) < 0.4).astype(np.int64)
    else:
        ql, gl = rng.integers(0, C, Qn), rng.integers(0, C, G)
        if t % 7 == 0:
            ql[-1] = C                                              # a query whose class is absent
    limits = [1, 3, 10, G, G + 5, -1]
    return D, aref.relevance(ql, gl), limits, bool(t % 2), int(rng.integers(0, 1000)) if t % 11 == 0 else 0


def test_rank_count_identity_equals_the_brute_force():
    rng = np.random.default_rng(20261019)
    for t in range(300):
        D, rel, limits, rf, base = _problem(rng, t)
        want = aref.evaluate(D, rel, limits, rf)
        got = aref.evaluate_by_rank_count(D, rel, limits, rf, base)
        for a, b, what in zip(got, want, ("S", "nrel", "total")):
            assert np.array_equal(a, b), (t, what)


def test_sign_codes_rank_as_hamming():
    """for +-s query codes every weight is L = 2^P - 1, so D = L * Hamming exactly and the two rankings are one"""
    rng = np.random.default_rng(5)
    for nbit, bits in ((48, 4), (64, 8), (120, 8)):
        sign = np.where(rng.random((9, nbit)) < 0.5, -1.0, 1.0)
        codes = (sign * rng.uniform(0.1, 9.0, (9, 1))).astype(np.float32)
        g = wref.pack_sign(rng.standard_normal((77, nbit)).astype(np.float32))
        q = wref.pack_sign(codes)
        ham = (wref.bits_of(q)[:, None, :] ^ wref.bits_of(g)[None, :, :]).sum(-1).astype(np.int64)
        assert np.array_equal(aref.distances(codes, g, bits), ((1 << bits) - 1) * ham)


def test_the_header_and_the_binding_name_the_entries():
    from concepthash_amd import _lib
    header = open(os.path.join(ROOT, "include", "concepthash_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert "void *stream" in m.group(1)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(args) == m.group(1).count(",") + 1, name
    assert re.search(r"#define CH_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3
    from concepthash_amd import build
    assert "hamming_rankcount.hip" in build.SOURCES


def test_calculate_map_refuses_before_it_touches_a_gpu(monkeypatch):
    import utils.hashing as hashing

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(hashing, "_device", no_gpu)
    monkeypatch.setattr(hashing.rt, "pack_sign", no_gpu)
    db, te = torch.randn(6, 16), torch.randn(3, 16)
    dl, tl = torch.arange(6) % 2, torch.arange(3) % 2
    with pytest.raises(ValueError, match="rank"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="nearest")
    with pytest.raises(ValueError, match="tie bracket"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="asymmetric", tie_bracket=True)
    with pytest.raises(ValueError, match="radius"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="asymmetric", radii=[0, 2])
    with pytest.raises(ValueError, match="weight_bits"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="asymmetric", weight_bits=5)
    from concepthash_amd.distributed import RowShard
    shard = RowShard.__new__(RowShard)
    with pytest.raises(NotImplementedError, match="sharded"):
        hashing.calculate_mAP(shard, shard, te, tl, -1, rank="asymmetric")


def test_evaluate_weighted_checks_its_arguments_without_a_gpu():
    from concepthash_amd import retrieval as rt
    g = torch.zeros(5, 1, dtype=torch.int64)
    lab = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="words per code"):
        rt.evaluate_weighted(torch.zeros(3, 100), g, lab[:3], lab)
    with pytest.raises(ValueError, match="weight bits"):
        rt.evaluate_weighted(torch.zeros(3, 64), g, lab[:3], lab, bits=6)
    with pytest.raises(ValueError, match="k >= 1"):
        rt.evaluate_weighted(torch.zeros(3, 64), g, lab[:3], lab, ks=(0,))
    with pytest.raises(TypeError):
        rt.evaluate_weighted(torch.zeros(3, 64), g.to(torch.int32), lab[:3], lab)
    # no query or no gallery row: the shapes of `empty_result`, nothing is launched
    out = rt.evaluate_weighted(torch.zeros(0, 64), g, lab[:0], lab, R=[5, -1])
    assert out["mAP"] == [0.0, 0.0] and out["hits"].shape == (0, 3) and len(out["S"]) == 2 and out["total"].shape == (0,)
    out = rt.evaluate_weighted(torch.zeros(3, 64), g[:0], lab[:3], lab[:0])
    assert out["mAP"] == 0.0 and out["precisions"] == [0.0] * 3 and out["S"].shape == (3,) and out["hits"].shape == (3, 3)
    assert set(out) == {"mAP", "precisions", "recalls", "hits", "total", "S", "nrel", "ap"}
    assert rt.rank_seg_rows(70, 771) == 256 and rt.rank_seg_rows(5794, 5994) == 5994 and rt.rank_seg_rows(1, 10 ** 9) >= -(-10 ** 9 // 65535)


def test_val_yaml_composes_with_the_two_keys(tmp_path):
    import yaml
    import main_v2
    from concepthash_amd import config as cfglib
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yaml").write_text(yaml.safe_dump({"seed": 7, "model": {"nbit": 64}, "batch_size": 32, "exp": "hashing"}))
    base = ["logdir=" + str(run), "dataset=synthetic_cub200"]
    val = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", base, cwd=str(tmp_path))
    assert val.asymmetric_eval is False and val.weight_bits == 8
    assert "asymmetric_eval" in main_v2.LOOP_KEYS and "weight_bits" in main_v2.LOOP_KEYS
    on = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", base + ["asymmetric_eval=true", "weight_bits=4"], cwd=str(tmp_path))
    laid = main_v2._run_config(on, "validation", main_v2.EVAL_KEYS)
    assert laid.asymmetric_eval is True and laid.weight_bits == 4 and laid.exp == "validation" and laid.model.nbit == 64


@pytest.mark.parametrize("tie,concept,radii", [(False, False, None), (True, False, None), (False, True, None), (True, True, [0, 2])])
def test_asymmetric_evaluation_records_its_triple_beside_each_call(tmp_path, monkeypatch, tie, concept, radii):
    """experiments.asymmetric_eval.AsymmetricEvaluation around a stub evaluator and a stub metric: every whole-code call is followed by
    the same call under rank="asymmetric" (without the bracket and the radii), the triple lands beside the call's own key, the
    evaluators it extends still find what the Hamming call left behind, and the rebound names are restored."""
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.asymmetric_eval import AsymmetricEvaluation
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, tie_bracket=False, PRs=None, radii=None, rank="hamming", weight_bits=8, **k):
        seen.append((tuple(db_codes.shape), bool(tie_bracket), radii, rank, weight_bits))
        m = float(db_codes.sum() + test_codes.sum()) + (0.25 if rank == "asymmetric" else 0.0)
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
    ev = AsymmetricEvaluation.__new__(AsymmetricEvaluation)
    ev.config = _wrap({"asymmetric_eval": True, "weight_bits": 4, "hash_lookup_radii": radii, "concept_eval": concept, "compute_mAP": True,
                       "exp": "validation", "tie_bracket": tie, "sub_code_eval": False, "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    m = float(db.sum() + te.sum())
    assert res["mAP"] == m and res["mAP_asymmetric"] == m + 0.25 and res["mAP_asymmetric_bin"] == 2 * m + 0.25
    assert res["recalls_asymmetric"] == [m + 0.25] * 2 and res["precisions_asymmetric"] == [-m - 0.25] * 2 and res["weight_bits"] == 4
    whole = [s for s in seen if s[0] == (5, 12)]
    assert whole == [((5, 12), tie, radii, "hamming", 8), ((5, 12), False, None, "asymmetric", 4)] * 2
    assert all(s[3] == "hamming" for s in seen if s[0] != (5, 12)) and len(seen) == (10 if concept else 4)
    assert ("mAP_tie_low" in res) == tie and ("mAP_concept" in res) == concept and ("precisions_radius" in res) == (radii is not None)
    if tie:
        assert res["mAP_tie_low"] == m - 1 and res["mAP_tie_high_bin"] == 2 * m + 1      # the Hamming call's bracket, not None
    if radii:
        assert res["precisions_radius"] == [m, m + 2]
    assert json.load(open(tmp_path / "history.json")) == res
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    ev.config["asymmetric_eval"] = False                        # the key off: the evaluators below alone
    seen.clear()
    off = ev.main()
    assert "mAP_asymmetric" not in off and "weight_bits" not in off and all(s[3] == "hamming" for s in seen)
