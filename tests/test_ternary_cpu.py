"""No GPU: ternary codes (csrc/hamming_ternary.hip) -- the numpy reference of tests/ternary_ref.py against
itself and against the C oracle, the library's exports and host-side argument checks, `calculate_mAP(rank="ternary")` refusing what it
does not define before it touches a GPU, `TernaryEvaluation` around a stub metric, and the mask plane of `GalleryIndex`."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ternary_ref as tref
from conftest import ROOT

ENTRIES = ("ch_pack_ternary", "ch_ternary_dist", "ch_ternary_topk_workspace", "ch_ternary_topk", "ch_ternary_rank_collect",
           "ch_ternary_rank_count")


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the reference against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbit", [1, 48, 64, 120, 256])
def test_definition_equals_the_plane_identity(nbit):
    rng = np.random.default_rng(nbit)
    xq, xg = rng.standard_normal((9, nbit)).astype(np.float32), rng.standard_normal((41, nbit)).astype(np.float32)
    xg[3] = 0.0
    xq[1, ::2] = np.nan
    for margin in (0.0, 0.4, 1.5):
        tq, tg = tref.ternarise(xq, margin), tref.ternarise(xg, margin)
        K = tref.dist(tq, tg)
        assert np.array_equal(K, tref.dist_planes(tref.planes(tq), tref.planes(tg), nbit))
        assert K.min() >= 0 and K.max() <= 2 * nbit and np.all(K[:, 3] == nbit)
        # the packed form's two identities
        assert np.array_equal(tref.planes(tg)[:, 1], tref.confidence_mask(xg, margin))
        assert np.array_equal(tref.planes(tg)[:, 0], tref.pack_sign(xg) & tref.confidence_mask(xg, margin))


@pytest.mark.parametrize("nbit", [48, 64, 120, 256])
def test_sure_codes_rank_as_twice_the_hamming_distance(nbit):
    from oracle import hamming_oracle as ho
    rng = np.random.default_rng(7 + nbit)
    sign = lambda r: np.where(rng.random((r, nbit)) < 0.5, -1.0, 1.0)
    xq = (sign(6) * rng.uniform(0.6, 3.0, (6, nbit))).astype(np.float32)
    xg = (sign(50) * rng.uniform(0.6, 3.0, (50, nbit))).astype(np.float32)
    K = tref.dist(tref.ternarise(xq, 0.5), tref.ternarise(xg, 0.5))          # every |x| > margin: no zero on either side
    assert np.array_equal(K, 2 * ho.dist(ho.pack(xq), ho.pack(xg)).astype(np.int64))
    idx, dst = tref.topk(K, 7)
    oidx, odst = ho.topk(ho.pack(xq), ho.pack(xg), 7)
    assert np.array_equal(idx, oidx.astype(np.int64)) and np.array_equal(dst, 2 * odst.astype(np.int64))


def test_ternariser_edges():
    x = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, -0.5, 0.50001, -0.50001, 1e-30]], dtype=np.float32)
    assert tref.ternarise(x, 0.5).tolist() == [[0, 0, 0, 1, -1, 0, 0, 1, -1, 0]]      # the comparison is strict
    assert tref.ternarise(x, 0.0).tolist() == [[0, 0, 0, 1, -1, 1, -1, 1, -1, 1]]      # a code of exactly 0 is ternary 0, not "bit 0"


# ---- library surface -------------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_library_name_the_entries(lib):
    from concepthash_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "concepthash_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == m.group(1).count(",") + 1, name
        assert name.endswith("_workspace") or ("void *stream" in m.group(1) and res is _lib.c_int), name
    assert re.search(r"#define CH_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3 and lib.ch_abi_version() == 3
    assert "hamming_ternary.hip" in build.SOURCES


def test_entries_refuse_bad_arguments_on_the_host(lib):
    buf = (ctypes.c_char * 64)()                    # non-null, never dereferenced: every call below is refused before any launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.ch_last_error().decode()

    def topk(W=1, nbit=64, k=10, Qn=4, G=4):
        return lib.ch_ternary_topk(p, Qn, p, G, W, nbit, k, 0, p, p, p, 1 << 20, None)

    def collect(W=1, nbit=64, Qn=4, G=4, base=0, LW=0):
        return lib.ch_ternary_rank_collect(p, Qn, p, G, W, nbit, p, p, LW, base, None, p, p, None)

    def count(W=1, nbit=64, Qn=4, G=4, base=0, seg=256, cap=16):
        return lib.ch_ternary_rank_count(p, Qn, p, G, W, nbit, base, seg, p, p, cap, p, None)
    # pack: nbit and margin
    for nbit in (0, 257, -4):
        assert lib.ch_pack_ternary(p, 4, nbit, 0.5, p, None) == 2 and "pack_ternary" in err() and "nbit" in err()
    for margin in (-0.5, float("inf"), float("nan")):
        assert lib.ch_pack_ternary(p, 4, 64, margin, p, None) == 2 and "pack_ternary" in err() and "margin" in err()
    assert lib.ch_pack_ternary(p, -1, 64, 0.5, p, None) == 2 and "rows" in err()
    assert lib.ch_pack_ternary(None, 4, 64, 0.5, p, None) == 2 and "null" in err()
    # the distance matrix
    for W in (0, 9):
        assert lib.ch_ternary_dist(p, 4, p, 4, W, 64, p, None) == 2 and "ternary_dist" in err() and "W" in err()
    for nbit in (0, 65):
        assert lib.ch_ternary_dist(p, 4, p, 4, 1, nbit, p, None) == 2 and "ternary_dist" in err() and "nbit" in err()
    assert lib.ch_ternary_dist(p, -1, p, 4, 1, 64, p, None) == 2 and "negative" in err()
    assert lib.ch_ternary_dist(p, 4, None, 4, 1, 64, p, None) == 2 and "null" in err()
    # top-k: the contract of ch_hamming_topk, and nbit
    for W in (0, 9):
        assert topk(W=W) == 2 and "ternary_topk" in err() and "W" in err()
    for k in (0, 129, 1000):
        assert topk(k=k) == 2 and "ternary_topk" in err() and "k" in err()
    for nbit in (0, 65, -1):
        assert topk(nbit=nbit) == 2 and "ternary_topk" in err() and "nbit" in err()
    assert topk(Qn=-1) == 2 and "negative" in err()
    assert lib.ch_ternary_topk(p, 4, p, 4, 1, 64, 10, 0, p, p, p, 8, None) == 2 and "workspace" in err()
    assert lib.ch_ternary_topk(p, 4, p, 4, 1, 64, 10, 0, None, p, p, 1 << 20, None) == 2 and "null" in err()
    assert lib.ch_ternary_topk_workspace(4, 4, 9, 10) == 16 and lib.ch_ternary_topk_workspace(70, 771, 4, 128) >= 70 * 128 * 4
    # collect and count
    for fn, who in ((collect, "ternary_rank_collect"), (count, "ternary_rank_count")):
        for W in (0, 9):
            assert fn(W=W) == 2 and who in err() and "W" in err()
        for nbit in (0, 65):
            assert fn(nbit=nbit) == 2 and who in err() and "nbit" in err()
        assert fn(G=-1) == 2 and "negative" in err()
        assert fn(base=-1) == 2 and "g_index_base" in err()
        assert fn(base=(1 << 32) - 3) == 2 and "g_index_base" in err()
    assert collect(LW=-1) == 2 and "LW" in err()
    for seg in (0, -5):
        assert count(seg=seg) == 2 and "seg_rows" in err()
    for cap in (0, 8193):
        assert count(cap=cap) == 2 and "list_cap" in err()
    assert count(G=1 << 30, seg=1) == 2 and "segments" in err()


def test_python_entries_check_their_arguments_without_a_gpu():
    from concepthash_amd import retrieval as rt
    q3, g3 = torch.zeros(3, 2, 2, dtype=torch.int64), torch.zeros(5, 2, 2, dtype=torch.int64)
    lab = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(TypeError, match="2, W"):
        rt.ternary_dist(q3[:, 0], g3, 100)
    with pytest.raises(TypeError):
        rt.ternary_topk(q3.to(torch.int32), g3, 100, 3)
    with pytest.raises(ValueError, match="words per plane"):
        rt.ternary_topk(q3[:, :, :1], g3, 64, 3)
    with pytest.raises(ValueError, match="nbit"):
        rt.ternary_dist(q3, g3, 129)
    with pytest.raises(ValueError, match="k >= 1"):
        rt.evaluate_ternary(q3, g3, 100, lab[:3], lab, ks=(0,))
    for bad in (None, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="margin"):
            rt.pack_ternary(torch.zeros(2, 8), bad)
    out = rt.evaluate_ternary(q3[:0], g3, 100, lab[:0], lab, R=[5, -1])
    assert out["mAP"] == [0.0, 0.0] and out["hits"].shape == (0, 3) and len(out["S"]) == 2
    out = rt.evaluate_ternary(q3, g3[:0], 100, lab[:3], lab[:0])
    assert set(out) == {"mAP", "precisions", "recalls", "hits", "total", "S", "nrel", "ap"} and out["S"].shape == (3,)


# ---- calculate_mAP ---------------------------------------------------------------------------------------------------------------
def test_calculate_map_refuses_before_it_touches_a_gpu(monkeypatch):
    import utils.hashing as hashing

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(hashing, "_device", no_gpu)
    monkeypatch.setattr(hashing.rt, "pack_sign", no_gpu)
    monkeypatch.setattr(hashing.rt, "pack_ternary", no_gpu)
    assert "ternary" in hashing.RANKS
    db, te = torch.randn(6, 16), torch.randn(3, 16)
    dl, tl = torch.arange(6) % 2, torch.arange(3) % 2
    with pytest.raises(ValueError, match="margin"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="ternary")
    with pytest.raises(ValueError, match="margin"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="ternary", margin=-0.25)
    with pytest.raises(ValueError, match="tie bracket"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="ternary", margin=0.3, tie_bracket=True)
    with pytest.raises(ValueError, match="radius"):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="ternary", margin=0.3, radii=[0, 2])
    from concepthash_amd.distributed import RowShard
    shard = RowShard.__new__(RowShard)
    with pytest.raises(NotImplementedError, match="sharded"):
        hashing.calculate_mAP(shard, shard, te, tl, -1, rank="ternary", margin=0.3)
    # threshold and dist_metric are what they were; the threshold message points at the ranking that is built
    with pytest.raises(NotImplementedError, match=r'rank="ternary", margin='):
        hashing.calculate_mAP(db, dl, te, tl, -1, threshold=0.5)
    with pytest.raises(NotImplementedError):
        hashing.calculate_mAP(db, dl, te, tl, -1, rank="ternary", margin=0.3, dist_metric="euclidean")


def test_calculate_map_hands_both_code_sets_to_the_ternary_evaluation(monkeypatch):
    import utils.hashing as hashing
    seen = []

    class FakeRt:
        check_margin = staticmethod(hashing.rt.check_margin)
        WEIGHT_BITS = hashing.rt.WEIGHT_BITS

        @staticmethod
        def pack_ternary(codes, margin):
            seen.append(("pack", tuple(codes.shape), margin))
            return codes

        @staticmethod
        def evaluate_ternary(q3, g3, nbit, ql, gl, **k):
            seen.append(("evaluate", tuple(q3.shape), tuple(g3.shape), nbit, k))
            return {"mAP": 0.5, "recalls": [0.1], "precisions": [0.2]}
    monkeypatch.setattr(hashing, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(hashing, "rt", FakeRt)
    db, te = torch.randn(6, 16), torch.randn(3, 16)
    out = hashing.calculate_mAP(db, torch.arange(6) % 2, te, torch.arange(3) % 2, 50, PRs=[5], rank="ternary", margin=0.25,
                                remove_first_retrieved=True, skip_queries_without_relevant=True)
    assert out == (0.5, [0.1], [0.2])
    assert seen[:2] == [("pack", (6, 16), 0.25), ("pack", (3, 16), 0.25)]
    assert seen[2] == ("evaluate", (3, 16), (6, 16), 16, dict(R=50, ks=[5], remove_first=True, skip_queries_without_relevant=True))


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
    assert val.ternary_eval is False and val.ternary_margin is None
    assert "ternary_eval" in main_v2.LOOP_KEYS and "ternary_margin" in main_v2.LOOP_KEYS
    on = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", base + ["ternary_eval=true", "ternary_margin=0.3"], cwd=str(tmp_path))
    laid = main_v2._run_config(on, "validation", main_v2.EVAL_KEYS)
    assert laid.ternary_eval is True and laid.ternary_margin == 0.3 and laid.exp == "validation"
    search = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", base + ["rank=ternary", "index_margin=0.2"], cwd=str(tmp_path))
    assert search.index_margin == 0.2 and "index_margin" in main_v2.SEARCH_KEYS and all(k in search for k in main_v2.SEARCH_KEYS)


@pytest.mark.parametrize("tie,concept,radii,asym", [(False, False, None, False), (True, False, None, True), (False, True, None, False),
                                                    (True, True, [0, 2], True)])
def test_ternary_evaluation_records_its_triple_beside_each_call(tmp_path, monkeypatch, tie, concept, radii, asym):
    """experiments.ternary_eval.TernaryEvaluation around a stub evaluator and a stub metric: every whole-code call is followed by the same
    call under rank="ternary" (without the bracket and the radii), the triple lands beside the call's own key, the evaluators it extends
    still find what the Hamming call left behind, the asymmetric call is not repeated, and the rebound names are restored."""
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.ternary_eval import TernaryEvaluation
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, tie_bracket=False, PRs=None, radii=None, rank="hamming", weight_bits=8,
               margin=None, **k):
        seen.append((tuple(db_codes.shape), bool(tie_bracket), radii, rank, margin))
        m = float(db_codes.sum() + test_codes.sum()) + {"hamming": 0.0, "asymmetric": 0.25, "ternary": 0.5}[rank]
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
    ev = TernaryEvaluation.__new__(TernaryEvaluation)
    ev.config = _wrap({"ternary_eval": True, "ternary_margin": 2.5, "asymmetric_eval": asym, "weight_bits": 4, "hash_lookup_radii": radii,
                       "concept_eval": concept, "compute_mAP": True, "exp": "validation", "tie_bracket": tie, "sub_code_eval": False,
                       "text_eval": False, "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    m = float(db.sum() + te.sum())
    assert res["mAP"] == m and res["mAP_ternary"] == m + 0.5 and res["mAP_ternary_bin"] == 2 * m + 0.5
    assert res["recalls_ternary"] == [m + 0.5] * 2 and res["precisions_ternary"] == [-m - 0.5] * 2 and res["ternary_margin"] == 2.5
    assert "recalls_ternary_bin" in res and "precisions_ternary_bin" in res
    # the zero share of the LAST whole-code call (db * 2, te * 2), database first
    want = [1.0 - float(((db * 2).abs() > 2.5).double().mean()), 1.0 - float(((te * 2).abs() > 2.5).double().mean())]
    assert res["ternary_zero_share"] == want and 0.0 < want[0] < 1.0 and 0.0 < want[1] < 1.0
    whole = [s for s in seen if s[0] == (5, 12)]
    per_call = [((5, 12), tie, radii, "hamming", None), ((5, 12), False, None, "ternary", 2.5)] + \
        ([((5, 12), False, None, "asymmetric", None)] if asym else [])
    assert whole == per_call * 2
    assert all(s[3] == "hamming" for s in seen if s[0] != (5, 12)) and len(seen) == len(whole) + (6 if concept else 0)
    assert ("mAP_tie_low" in res) == tie and ("mAP_concept" in res) == concept and ("precisions_radius" in res) == (radii is not None)
    assert ("mAP_asymmetric" in res) == asym
    if tie:
        assert res["mAP_tie_low"] == m - 1 and res["mAP_tie_high_bin"] == 2 * m + 1      # the Hamming call's bracket, not None
    if radii:
        assert res["precisions_radius"] == [m, m + 2]
    if asym:
        assert res["mAP_asymmetric"] == m + 0.25 and res["mAP_asymmetric_bin"] == 2 * m + 0.25
    assert json.load(open(tmp_path / "history.json")) == res
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    ev.config["ternary_eval"] = False                           # the key off: the evaluators below alone
    seen.clear()
    off = ev.main()
    assert "mAP_ternary" not in off and "ternary_margin" not in off and all(s[3] != "ternary" for s in seen)
    ev.config["ternary_eval"], ev.config["ternary_margin"] = True, None
    with pytest.raises(ValueError, match="ternary_margin"):
        ev.main()


# ---- the index -------------------------------------------------------------------------------------------------------------------
def _index(with_mask, nbit=120, Q=3, G=7):
    from concepthash_amd.search import GalleryIndex
    g = torch.Generator().manual_seed(5)
    W = (nbit + 63) // 64
    codes = torch.randint(-2 ** 62, 2 ** 62, (G, W), generator=g, dtype=torch.int64)
    mask = torch.randint(-2 ** 62, 2 ** 62, (G, W), generator=g, dtype=torch.int64) if with_mask else None
    return GalleryIndex(codes, nbit, Q, labels=torch.arange(G) % 3, transform={"resize": 256, "crop": 224, "norm": 2},
                        fingerprint={"file": "best.pth", "size": 11, "sha256": "ab" * 32}, mask=mask, margin=0.25 if with_mask else None)


@pytest.mark.parametrize("with_mask", [True, False])
def test_gallery_index_round_trip_with_and_without_the_mask_plane(tmp_path, with_mask):
    from concepthash_amd.search import GalleryIndex
    a = _index(with_mask)
    path = str(tmp_path / "index.pth")
    a.save(path)
    raw = torch.load(path, map_location="cpu")
    old = {"format", "codes", "nbit", "ncontext", "labels", "paths", "data_root", "mean", "transform", "fingerprint"}
    assert raw["format"] == 1 and set(raw) == (old | {"mask", "margin"} if with_mask else old)
    b = GalleryIndex.load(path, fingerprint=dict(a.fingerprint), nbit=120)
    assert torch.equal(a.codes, b.codes) and b.margin == a.margin
    assert (b.mask is None) == (not with_mask) and (b.mask is None or torch.equal(a.mask, b.mask))
    c = b.to("cpu")
    assert c.margin == a.margin and (c.mask is None) == (not with_mask)


def test_an_index_file_written_without_the_plane_still_loads_and_names_what_ternary_needs(tmp_path):
    from concepthash_amd.search import GalleryIndex
    a = _index(False)
    path = str(tmp_path / "index.pth")
    torch.save({"format": 1, "codes": a.codes, "nbit": a.nbit, "ncontext": a.ncontext, "labels": a.labels, "paths": None, "data_root": None,
                "mean": None, "transform": a.transform, "fingerprint": a.fingerprint}, path)         # the file of before, key for key
    b = GalleryIndex.load(path, fingerprint=dict(a.fingerprint), nbit=120)
    assert b.mask is None and b.margin is None and torch.equal(b.codes, a.codes)
    with pytest.raises(ValueError, match=r"index_margin.*rebuild_index=true"):
        b.search(torch.zeros(2, 120), 3, rank="ternary", margin=0.1)
    m = _index(True)
    with pytest.raises(ValueError, match="not built"):
        m.search(torch.zeros(2, 120), 129, rank="ternary", margin=0.1)
    with pytest.raises(ValueError, match="margin"):
        m.search(torch.zeros(2, 120), 3, rank="ternary", margin=-1.0)
    with pytest.raises(ValueError, match="mask"):
        GalleryIndex(a.codes, 120, 3, mask=a.codes[:3], margin=0.1)
    with pytest.raises(ValueError, match="margin"):
        GalleryIndex(a.codes, 120, 3, mask=a.codes)
