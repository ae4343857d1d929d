"""GPU: evaluation under the weighted (asymmetric) ranking -- `retrieval.evaluate_weighted` (csrc/hamming_rankcount.hip: collect, rank
count, AP from bins) against the brute-force numpy reference of tests/asymmetric_eval_ref.py, at the smallest shapes that reach every
path of the kernels; against the Hamming evaluator where the two rankings are one; against the ranking `hamming_topk_weighted` serves;
`utils.hashing.calculate_mAP(rank="asymmetric")` and `main_v2.py --config-name val.yaml asymmetric_eval=true` on a synthetic run
directory.  All arithmetic is integer: every comparison of S, nrel, hits and total is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import asymmetric_eval_ref as aref
import weighted_topk_ref as wref
from conftest import ROOT

pytestmark = pytest.mark.gpu

QN = 70
G_SIZES = (1, 63, 771)    # 771: three 256-row segments and a 3-row tail
KS = (1, 5, 10)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(out, want, Rs, ks, limits, what):
    """out: evaluate_weighted(R=list Rs, ks); want = (S, nrel, total) of the reference under `limits` = Rs + ks"""
    S, nrel, total = want
    for i in range(len(Rs)):
        assert np.array_equal(out["S"][i].cpu().numpy().view(np.uint64), S[i]), (what, "S", Rs[i])
        assert np.array_equal(out["nrel"][i].cpu().numpy(), nrel[i]), (what, "nrel", Rs[i])
    for t in range(len(ks)):
        assert np.array_equal(out["hits"][:, t].cpu().numpy(), nrel[len(Rs) + t]), (what, "hits", ks[t])
    assert np.array_equal(out["total"].cpu().numpy(), total), (what, "total")
    ap = np.where(nrel[0] > 0, S[0].astype(np.float64) / (np.maximum(nrel[0], 1) * 2.0 ** 32), 0.0)
    assert abs(out["mAP"][0] - ap.mean()) < 1e-12, (what, "mAP")


def _gallery(rng, G, nbit):
    """real-valued gallery codes with many duplicated rows, so that equal D is common"""
    c = rng.standard_normal((G, nbit)).astype(np.float32)
    if G > 3:
        c[rng.integers(0, G, G // 2)] = c[rng.integers(0, G, G // 2)]
    return c


# ---- the grid against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("remove_first", [False, True])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("nbit", [48, 64, 120, 256])
def test_grid_equals_the_reference(dev, nbit, bits, remove_first):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(7000 + nbit + bits + int(remove_first))
    W = (nbit + 63) // 64
    codes = rng.standard_normal((QN, nbit)).astype(np.float32)
    codes[0] = 0.0                                                   # every D = 0: the ranking is by index
    codes[1, 1], codes[1, 7], codes[1, nbit - 1] = np.nan, np.inf, -np.inf
    mask = np.full((QN, W), ~np.uint64(0), np.uint64)                # bits past nbit set: they must not count
    mask[2] = rt.concept_mask(nbit, 4, [1, 3]).numpy().view(np.uint64)
    ql = rng.integers(0, 7, QN)
    ql[5] = 7                                                        # a class the gallery does not hold
    for G in G_SIZES:
        gc = _gallery(rng, G, nbit)
        g = wref.pack_sign(gc)
        gl = rng.integers(0, 7, G)
        D = wref.dist(wref.pack_sign(codes), g, wref.weights(codes, bits, mask))
        rel = aref.relevance(ql, gl)
        Rs = [1, 5, 50, G, G + 9, -1]
        want = aref.evaluate(D, rel, Rs + list(KS), remove_first)
        args = (_t(codes, dev), _t(g, dev), _t(ql, dev), _t(gl, dev))
        for seg in (None, max(1, G // 4 + 1)):                       # the default segmentation, and at least 3 segments adding into the bins
            out = rt.evaluate_weighted(*args, bits=bits, mask=_t(mask, dev), R=Rs, ks=KS, remove_first=remove_first, seg_rows=seg)
            _check(out, want, Rs, KS, Rs + list(KS), (nbit, bits, remove_first, G, seg))
        assert int(out["total"][5]) == 0 and int(out["S"][-1][5]) == 0 and int(out["nrel"][-1][5]) == 0
        many = list(range(1, 17)) + [-1]                             # 17 distinct limits: two launches of the AP kernel, one scan
        out = rt.evaluate_weighted(*args, bits=bits, mask=_t(mask, dev), R=many, ks=(), remove_first=remove_first)
        _check(out, aref.evaluate(D, rel, many, remove_first), many, (), many, (nbit, bits, remove_first, G, "17 limits"))
        one = rt.evaluate_weighted(*args, bits=bits, mask=_t(mask, dev), R=-1, ks=KS, remove_first=remove_first)   # a single R: no lists
        assert torch.equal(one["S"], out["S"][-1]) and torch.equal(one["nrel"], out["nrel"][-1]) and isinstance(one["mAP"], float)


# ---- lists longer than the LDS-resident capacity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("remove_first", [False, True])
def test_long_lists_are_searched_in_global_memory_with_the_same_result(dev, remove_first):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(81)
    nbit, G = 64, 771
    codes = rng.standard_normal((QN, nbit)).astype(np.float32)
    gc = _gallery(rng, G, nbit)
    gl = np.where(np.arange(G) < 600, 0, rng.integers(1, 7, G))      # one class holds 600 of the 771 rows
    rng.shuffle(gl)
    ql = rng.integers(0, 7, QN)
    ql[:20] = 0
    g = wref.pack_sign(gc)
    Rs = [1, 5, 50, G, -1]
    want = aref.evaluate(aref.distances(codes, g, 8), aref.relevance(ql, gl), Rs + list(KS), remove_first)
    args = (_t(codes, dev), _t(g, dev), _t(ql, dev), _t(gl, dev))
    for cap, seg in ((None, None), (8, None), (8, 200), (1, 771)):   # cap 8: every query's list (>= 20 keys) is read from global memory
        out = rt.evaluate_weighted(*args, bits=8, R=Rs, ks=KS, remove_first=remove_first, list_cap=cap, seg_rows=seg)
        _check(out, want, Rs, KS, Rs + list(KS), ("long lists", cap, seg))


# ---- multi-hot labels ----------------------------------------------------------------------------------------------------------------

def test_multi_hot_labels(dev):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(82)
    nbit, G, C = 120, 771, 70                                        # 70 classes: two label words

    def hot(rows):
        lab = np.zeros((rows, C), np.int64)
        for i in range(rows):
            lab[i, rng.choice(C, int(rng.integers(1, 4)), replace=False)] = 1
        return lab
    codes = rng.standard_normal((QN, nbit)).astype(np.float32)
    g = wref.pack_sign(_gallery(rng, G, nbit))
    ql, gl = hot(QN), hot(G)
    assert rt.prepare_labels(torch.from_numpy(ql), torch.from_numpy(gl))[2] == 2
    Rs = [10, G, -1]
    for rf in (False, True):
        want = aref.evaluate(aref.distances(codes, g, 4), aref.relevance(ql, gl), Rs + list(KS), rf)
        out = rt.evaluate_weighted(_t(codes, dev), _t(g, dev), _t(ql, dev), _t(gl, dev), bits=4, R=Rs, ks=KS, remove_first=rf, seg_rows=256)
        _check(out, want, Rs, KS, Rs + list(KS), ("multi-hot", rf))


# ---- self-retrieval ------------------------------------------------------------------------------------------------------------------

def test_self_retrieval_drops_rank_one(dev):
    """queries = gallery rows, remove_first: the dropped row is rank 1 of (D, index) -- the query's own row, or an exact duplicate of it
    at a lower index, whatever its label"""
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(83)
    nbit, G = 64, 300
    gc = rng.standard_normal((G, nbit)).astype(np.float32)
    gl = rng.integers(0, 5, G)
    gc[200], gc[201], gc[202] = gc[10], gc[11], gc[12]               # duplicates of rows 200.. at lower indices ...
    gl[10], gl[200] = 1, 1                                           # ... with the query's label,
    gl[11], gl[201] = 2, 3                                           # ... with another one,
    gl[12], gl[202] = 4, 4
    gc[13] = gc[202]                                                 # ... and two of them
    gl[13] = 0
    sel = np.concatenate([np.arange(0, 64), np.arange(195, 205)])
    codes, ql = gc[sel], gl[sel]
    g = wref.pack_sign(gc)
    Rs = [1, 10, G - 1, -1]
    D, rel = aref.distances(codes, g, 8), aref.relevance(ql, gl)
    assert (D[np.arange(len(sel)), sel] == 0).all()
    want = aref.evaluate(D, rel, Rs + list(KS), True)
    out = rt.evaluate_weighted(_t(codes, dev), _t(g, dev), _t(ql, dev), _t(gl, dev), bits=8, R=Rs, ks=KS, remove_first=True)
    _check(out, want, Rs, KS, Rs + list(KS), "self-retrieval")


# ---- where the two rankings are one --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("remove_first", [False, True])
@pytest.mark.parametrize("nbit", [64, 120])
def test_sign_codes_give_the_hamming_evaluation(dev, nbit, remove_first):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(84 + nbit)
    G = 771
    sign = np.where(rng.random((QN, nbit)) < 0.5, -1.0, 1.0)
    codes = (sign * rng.uniform(0.05, 20.0, (QN, 1))).astype(np.float32)     # +-s_i: every weight is 2^P - 1
    g = _t(wref.pack_sign(_gallery(rng, G, nbit)), dev)
    ql, gl = _t(rng.integers(0, 7, QN), dev), _t(rng.integers(0, 7, G), dev)
    c = _t(codes, dev)
    for R in (-1, 20, [1, 20, G, -1]):
        ham = rt.evaluate(rt.pack_sign(c), g, ql, gl, R=R, ks=KS, remove_first=remove_first)
        for bits in (4, 8):
            out = rt.evaluate_weighted(c, g, ql, gl, bits=bits, R=R, ks=KS, remove_first=remove_first)
            for key in ("S", "nrel"):
                a, b = (out[key], ham[key]) if isinstance(R, list) else ([out[key]], [ham[key]])
                assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), (key, R, bits)
            assert torch.equal(out["hits"], ham["hits"]) and torch.equal(out["total"], ham["total"]), (R, bits)
            assert out["mAP"] == ham["mAP"] and out["precisions"] == ham["precisions"] and out["recalls"] == ham["recalls"]


# ---- the ranking that is served ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [4, 8])
def test_hits_equal_the_relevant_rows_of_the_served_top_k(dev, bits):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(85)
    nbit, G = 64, 771
    codes = _t(rng.standard_normal((QN, nbit)).astype(np.float32), dev)
    g = _t(wref.pack_sign(_gallery(rng, G, nbit)), dev)
    ql, gl = _t(rng.integers(0, 7, QN), dev), _t(rng.integers(0, 7, G), dev)
    ks = (1, 10, 128)
    out = rt.evaluate_weighted(codes, g, ql, gl, bits=bits, ks=ks)
    planes, _ = rt.weight_planes(codes, bits)
    for t, k in enumerate(ks):
        idx, _ = rt.hamming_topk_weighted(rt.pack_sign(codes), planes, g, k)
        assert torch.equal(out["hits"][:, t].long(), (gl[idx] == ql[:, None]).sum(1)), k


# ---- CUB width -----------------------------------------------------------------------------------------------------------------------

def test_cub_width_against_the_reference(dev):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(86)
    Qn, G, nbit, C = 512, 5994, 64, 200
    centres = np.where(rng.random((C, nbit)) < 0.5, -1.0, 1.0)
    ql, gl = rng.integers(0, C, Qn), np.arange(G) % C
    codes = aref.clustered_codes(rng, Qn, nbit, ql, centres)
    g = wref.pack_sign(aref.clustered_codes(rng, G, nbit, gl, centres))
    Rs = [100, -1]
    want = aref.evaluate(aref.distances(codes, g, 8), aref.relevance(ql, gl), Rs + list(KS))
    out = rt.evaluate_weighted(_t(codes, dev), _t(g, dev), _t(ql, dev), _t(gl, dev), bits=8, R=Rs, ks=KS)
    _check(out, want, Rs, KS, Rs + list(KS), "CUB width")


# ---- surface -------------------------------------------------------------------------------------------------------------------------

def test_calculate_map_asymmetric_equals_evaluate_weighted(dev):
    from concepthash_amd import retrieval as rt
    from utils import hashing
    rng = np.random.default_rng(87)
    db, te = torch.from_numpy(_gallery(rng, 300, 64)), torch.from_numpy(rng.standard_normal((40, 64)).astype(np.float32))
    dl, tl = torch.from_numpy(rng.integers(0, 6, 300)), torch.from_numpy(rng.integers(0, 6, 40))
    for bits, R, rf in ((8, -1, False), (4, [10, -1], True)):
        mAP, recalls, precisions = hashing.calculate_mAP(db, torch.nn.functional.one_hot(dl, 6), te, torch.nn.functional.one_hot(tl, 6), R,
                                                         PRs=[1, 5], remove_first_retrieved=rf, rank="asymmetric", weight_bits=bits)
        out = rt.evaluate_weighted(te.to(dev), rt.pack_sign(db.to(dev)), tl.to(dev), dl.to(dev), bits=bits, R=R, ks=(1, 5), remove_first=rf)
        assert mAP == out["mAP"] and recalls == out["recalls"] and precisions == out["precisions"]
        assert hashing.last_tie_bracket is None and hashing.last_hash_lookup is None
    plain = hashing.calculate_mAP(db, dl, te, tl, -1, PRs=[1, 5])
    assert plain == hashing.calculate_mAP(db, dl, te, tl, -1, PRs=[1, 5], rank="hamming")


def test_main_v2_validation_with_asymmetric_eval(tmp_path, dev):
    """`main_v2.py --config-name val.yaml ... asymmetric_eval=true` on the synthetic run directory of tests/test_surface_gpu.py: the three
    keys are in history.json, equal a direct call on the saved codes, and the Hamming keys equal those of a run without the option."""
    from concepthash_amd import retrieval as rt
    logdir = str(tmp_path / "run")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["dataset=synthetic_cub200", "dataset.limit=96", "data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True, env=env, cwd=str(tmp_path))

    def run(extra, name):
        ev = str(tmp_path / name)
        subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "--config-name", "val.yaml", "logdir=" + logdir, "batch_size=32",
                        "save_code=True", "R=[10,-1]", "eval_logdir=" + ev] + common + extra, check=True, env=env, cwd=str(tmp_path))
        return json.load(open(os.path.join(ev, "history.json"))), torch.load(os.path.join(ev, "outputs.pth"))
    plain, _ = run([], "ev0")
    hist, outs = run(["asymmetric_eval=true", "weight_bits=4"], "ev1")
    assert not any("asymmetric" in k for k in plain) and "weight_bits" not in plain
    for key in ("mAP", "recalls", "precisions"):
        assert hist[key] == plain[key], key
    assert {k for k in hist if k not in plain} == {"mAP_asymmetric", "recalls_asymmetric", "precisions_asymmetric", "weight_bits"}
    db, te = outs["db"], outs["test"]
    out = rt.evaluate_weighted(te["codes"].to(dev), rt.pack_sign(db["codes"].to(dev)), te["labels"].to(dev), db["labels"].to(dev), bits=4,
                               R=[10, -1], ks=(1, 5, 10))
    assert hist["weight_bits"] == 4 and hist["mAP_asymmetric"] == out["mAP"]
    assert hist["recalls_asymmetric"] == out["recalls"] and hist["precisions_asymmetric"] == out["precisions"]
