"""GPU: the learned rotation ("learned rotation"; csrc/itq.hip) against the fp64 reference tests/itq_ref.py --
exact inputs compared for equality, general inputs inside derived bounds with no sign decision left out, the consistency of the step
and the rotate kernels, the fit on planted and on unstructured data, and the rotation in `GalleryIndex`, `exp=search rotate=itq` and
`exp=validation itq_eval=true`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import itq_ref as ir
from conftest import ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # the unit roundoff of fp32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _step(V, R, s, dev, seg_rows=None):
    from concepthash_amd import retrieval as rt
    M, l1, qerr = rt.itq_step(_t(V, dev), _t(R, dev), V.shape[1] // s, seg_rows)
    return M.cpu().numpy(), l1, qerr


def _rotate(V, R, s, dev):
    from concepthash_amd import retrieval as rt
    return rt.rotate_codes(_t(V, dev), _t(R, dev), V.shape[1] // s).cpu().numpy()


# ---- 1. exact inputs -----------------------------------------------------------------------------------------------------------------
EXACT = [(515, 64, 16), (515, 64, 64), (300, 256, 16), (300, 256, 256), (130, 16, 4), (1, 64, 16), (513, 64, 16)]


@pytest.mark.parametrize("G,n,s", EXACT)
def test_exact_inputs_give_the_reference_exactly(G, n, s, dev):
    """R_b = H_s / sqrt(s), V = odd multiples of 2^-8 in [-2, 2]: every partial sum of z (|z| <= 2 sqrt(s), multiples of 2^-12) and of M
    (|M| <= 2 G, multiples of 2^-8) is exact in fp32 in any order, so rotate and M must EQUAL the fp64 reference, whatever the
    segmentation; z has exact zeros, which pins the sign rule.  L1 and the cosine sum: a row's |z| and z^2 are added in fp32 (n terms,
    z^2 rounded once more) before fp64 takes over, so they match within n 2^-24 relative."""
    V, R = ir.exact_case(G, n, s, seed=G + n + s)
    M_ref, l1_ref, cos_ref, qerr_ref, z_ref = ir.step(V, R)
    if G >= 4:
        assert (z_ref == 0).any()
    z = _rotate(V, R, s, dev)
    assert z.dtype == np.float32 and np.array_equal(z.astype(np.float64), z_ref)
    for seg in (None, 256):
        M, l1, qerr = _step(V, R, s, dev, seg)
        assert M.dtype == np.float64 and M.shape == (n, s)
        assert np.array_equal(M, M_ref), (seg, np.abs(M - M_ref).max())
        assert abs(l1 - l1_ref) <= n * U * l1_ref, (seg, l1, l1_ref)
        cos = (1.0 - qerr) * G
        assert abs(cos - cos_ref) <= n * U * cos_ref + 1e-12 * G, (seg, cos, cos_ref)


# ---- 2. general inputs ---------------------------------------------------------------------------------------------------------------
GENERAL_G = 2000


@pytest.fixture(scope="module")
def general():
    made = {}

    def get(n, s):
        if (n, s) not in made:
            made[n, s] = ir.general_case(GENERAL_G, n, s, seed=7 * n + s)
        return made[n, s]
    return get


@pytest.mark.parametrize("n,s", [(64, 16), (64, 64), (256, 256), (48, 12)])
def test_general_inputs_stay_inside_the_derived_bounds(n, s, general, dev):
    """Gaussian V, R from a QR; every row has min_j |z_ij| >= tau = 4 n 2^-24 max_i |v_i|_1 max |R| under the fp64 chain, chosen before
    the GPU sees anything, so NO sign decision is left out (asserted).
    rotate: an fmaf chain of s terms from 0 differs from the exact sum by at most gamma_s sum_l |v_l r_l| <= s 2^-24 (1 + 1e-4) sum_l |v_l r_l|
    -- below tau, so every fp32 sign is the reference's.
    M: with equal signs, entry (j, l) is a sum of +-V_il whose fp32 part is a chain acc = fmaf(+-1, V_il, acc) over the c rows of a segment
    (c = min(seg_rows, G) <= 4096; the chain inside a row belongs to z, not to M), then fp64 over the segments (2^-53 per term:
    nothing): |M - M_ref| <= gamma_c sum_i |V_il| <= (c + 2) 2^-24 sum_i |V_il|."""
    V, R, tau = general(n, s)
    G = V.shape[0]
    V64, R64 = V.astype(np.float64), R.astype(np.float64)
    M_ref, l1_ref, cos_ref, _, z_ref = ir.step(V, R)
    left_out = int((np.abs(z_ref) < tau).sum())
    assert G == GENERAL_G and left_out == 0
    absz = np.concatenate([np.abs(V64[:, b * s:(b + 1) * s]) @ np.abs(R64[b * s:(b + 1) * s]) for b in range(n // s)], axis=1)
    z = _rotate(V, R, s, dev).astype(np.float64)
    excess = np.abs(z - z_ref) - s * U * (1 + 1e-4) * absz
    print(f"rotate {n}/{s}: max |z - z_ref| = {np.abs(z - z_ref).max():.3e}, largest bound excess {excess.max():.3e}, tau {tau:.3e}")
    assert excess.max() <= 0
    assert np.array_equal(z > 0, z_ref > 0)
    colsum = np.concatenate([np.tile(np.abs(V64[:, b * s:(b + 1) * s]).sum(0), (s, 1)) for b in range(n // s)])   # [n, s]: sum_i |V_il| of j's block
    for seg, c in ((None, 64), (4096, G), (300, 300)):
        M, l1, qerr = _step(V, R, s, dev, seg)
        excess = np.abs(M - M_ref) - (c + 2) * U * colsum
        print(f"M {n}/{s} seg {seg}: max |M - M_ref| = {np.abs(M - M_ref).max():.3e}, smallest bound {((c + 2) * U * colsum).min():.3e}")
        assert excess.max() <= 0, seg
        # the statistics follow the fp32 z: |z - z_ref| <= s u A (A = sum_l |v||r|, above), and a row's fp32 sums add n u relative.
        # L1: (s + n) u sum A.  Cosine c_i = l1_i / sqrt(n q_i), q_i = sum_j z_ij^2: |dc_i| <= c_i (d1_i + d2_i / 2) with
        # d1_i = (s + n) u sum_j A_ij / l1_i and d2_i = (2 s u sum_j |z_ij| A_ij + (n + 2) u q_i) / q_i (each z^2 is rounded once more).
        assert abs(l1 - l1_ref) <= (s + n) * U * (1 + 1e-4) * absz.sum()
        l1_i, q_i = np.abs(z_ref).sum(1), (z_ref * z_ref).sum(1)
        d1 = (s + n) * U * absz.sum(1) / l1_i
        d2 = (2 * s * U * (np.abs(z_ref) * absz).sum(1) + (n + 2) * U * q_i) / q_i
        cos_bound = float((l1_i / np.sqrt(n * q_i) * (d1 + d2 / 2)).sum()) * (1 + 1e-3)
        print(f"  cosine sum off by {abs((1.0 - qerr) * G - cos_ref):.3e}, bound {cos_bound:.3e}")
        assert abs((1.0 - qerr) * G - cos_ref) <= cos_bound
    # the signs the step used, decoded row by row: alone, M[j, l] = B_j V[l]
    for i in range(0, G, G // 8):
        M1, _, _ = _step(V[i:i + 1], R, s, dev)
        lead = np.abs(V64[i].reshape(n // s, s)).argmax(1)                       # the largest entry of each block of the row
        B = np.array([np.sign(M1[j, lead[j // s]] * V64[i, (j // s) * s + lead[j // s]]) for j in range(n)])
        assert np.array_equal(B, ir.sign(z_ref[i])), i


def test_default_segment_rule_of_the_general_test(dev):
    """the c = 64 the bound above uses under seg_rows=None: the library's workspace for 2,000 rows is that of 32 segments of 64 rows"""
    from concepthash_amd import _lib
    lib = _lib.load()
    assert lib.ch_itq_step_workspace(GENERAL_G, 64, 16, 0) == lib.ch_itq_step_workspace(GENERAL_G, 64, 16, 64) == 32 * (16 + 64 * 16 * 4) + 16


# ---- 3. consistency ------------------------------------------------------------------------------------------------------------------
def test_a_row_rotates_alone_as_in_a_batch_and_the_step_uses_those_signs(general, dev):
    V, R, _ = general(64, 16)
    V = V[:515]
    z = _rotate(V, R, 16, dev)
    for i in (0, 1, 63, 64, 255, 256, 514):
        assert np.array_equal(_rotate(V[i:i + 1], R, 16, dev)[0].view(np.uint32), z[i].view(np.uint32)), i
    # the step's signs are the signs of rotate's output: M from them in fp64 is inside the fp32 chain's bound of the step's M, a flipped
    # sign would move an entry by 2 |V_il|; and its L1 is the sum of |rotate's output| up to the row sums' rounding
    M, l1, _ = _step(V, R, 16, dev)
    B = ir.sign(z.astype(np.float64))
    V64 = V.astype(np.float64)
    M_rot = np.concatenate([B[:, b * 16:(b + 1) * 16].T @ V64[:, b * 16:(b + 1) * 16] for b in range(4)])
    colsum = np.concatenate([np.tile(np.abs(V64[:, b * 16:(b + 1) * 16]).sum(0), (16, 1)) for b in range(4)])
    assert (np.abs(M - M_rot) <= 66 * U * colsum).all()
    l1_rot = float(np.abs(z.astype(np.float64)).sum())
    assert abs(l1 - l1_rot) <= 64 * U * l1_rot
    M2, l12, q2 = _step(V, R, 16, dev)
    assert np.array_equal(M.view(np.uint64), M2.view(np.uint64)) and l1 == l12


def test_two_runs_are_bit_identical_at_every_segmentation(general, dev):
    V, R, _ = general(256, 256)
    for seg in (None, 4096, 300):
        a, b = _step(V, R, 256, dev, seg), _step(V, R, 256, dev, seg)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1:] == b[1:]


def test_library_refusals_and_empty_input(dev):
    from concepthash_amd import _lib, retrieval as rt
    lib = _lib.load()
    V, R = torch.zeros(8, 64, device=dev), torch.eye(16, device=dev).repeat(4, 1)
    M, st = torch.zeros(64, 16, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    ws = torch.zeros(1024, dtype=torch.int64, device=dev)
    p, sp = _lib.ptr, _lib.stream_ptr()
    for args, word in (((p(V), 8, 300, p(R), 4, 0), b"n must be in [1, 256]"), ((p(V), 8, 64, p(R), 5, 0), b"divide n"),
                       ((p(V), -1, 64, p(R), 16, 0), b"negative rows"), ((None, 8, 64, p(R), 16, 0), b"null pointer"),
                       ((p(V), 8, 64, p(R), 16, 5000), b"seg_rows")):
        assert lib.ch_itq_step(*args, p(M), p(st), p(ws), 8192, sp) == 2 and word in lib.ch_last_error(), word
    assert lib.ch_itq_step(p(V), 8, 64, p(R), 16, 0, p(M), p(st), p(ws), 8, sp) == 2 and b"workspace too small" in lib.ch_last_error()
    assert lib.ch_itq_rotate(p(V), 8, 64, None, 16, p(V), sp) == 2 and b"null pointer" in lib.ch_last_error()
    assert lib.ch_itq_rotate(p(V), 8, 64, p(R), 7, p(V), sp) == 2 and b"divide n" in lib.ch_last_error()
    assert lib.ch_itq_step(None, 0, 64, None, 16, 0, None, None, None, 0, sp) == 0 and lib.ch_itq_rotate(None, 0, 64, None, 16, None, sp) == 0
    M0, l1, qerr = rt.itq_step(V[:0], R, 4)
    assert tuple(M0.shape) == (64, 16) and float(M0.abs().max()) == 0 and (l1, qerr) == (0.0, 0.0)
    assert tuple(rt.rotate_codes(V[:0], R, 4).shape) == (0, 64)
    # a zero row contributes 1 to qerr and nothing to M
    M1, l1, qerr = rt.itq_step(V, R, 4)
    assert float(M1.abs().max()) == 0 and l1 == 0.0 and qerr == 1.0


# ---- 4. the fit on planted data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n,s", [(4096, 64, 16), (9000, 64, 64)])
def test_the_fit_recovers_a_planted_rotation_as_the_reference_does(G, n, s, dev):
    """X = B0 * a, a in (0.5, 1.5), V = X Q0^T with 30-degree Givens rotations inside each block.  The reference's fit is computed
    here; the GPU's may round M differently, never decide a sign differently (min |z| is about 0.4 along the way)."""
    from concepthash_amd import retrieval as rt
    V = ir.planted_case(G, n, s, seed=G)
    ref = ir.fit(V, s)
    assert ref["qerr_after"] < 0.3 * ref["qerr_before"]                                 # the construction has something to find
    fit = rt.fit_rotation(_t(V, dev), n // s)
    R = rt.compact_rotation(fit["R"], n // s).cpu().numpy().astype(np.float64)
    print(f"planted {G}x{n}/{s}: iters_run {fit['iters_run']} (ref {ref['iters_run']}), max |R - R_ref| {np.abs(R - ref['R']).max():.3e}, "
          f"qerr {fit['qerr_before']:.6f} -> {fit['qerr_after']:.6f} (ref {ref['qerr_after']:.6f})")
    assert fit["blocks"] == n // s and fit["R"].dtype == torch.float32 and tuple(fit["R"].shape) == (n, n)
    assert fit["iters_run"] <= ref["iters_run"] + 1
    assert np.abs(R - ref["R"]).max() <= 1e-5
    z = rt.rotate_codes(_t(V, dev), fit["R"], n // s).cpu().numpy()
    assert np.array_equal(z > 0, ir.chain(V, ref["R"]) > 0)
    assert abs(fit["qerr_after"] - ref["qerr_after"]) <= 1e-6
    assert abs(fit["qerr_before"] - ref["qerr_before"]) <= 1e-6 and len(fit["l1"]) >= fit["iters_run"] + 1


# ---- 5. the fit on unstructured data -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [16, 64])
def test_the_fit_is_monotone_on_unstructured_data(s, dev):
    from concepthash_amd import retrieval as rt
    V, _ = ir.clustered_case(5000, 64, seed=3)
    fit = rt.fit_rotation(_t(V, dev), 64 // s, iters=50)
    l1 = fit["l1"]
    print(f"clustered 5000x64/{s}: {len(l1)} passes, qerr {fit['qerr_before']:.5f} -> {fit['qerr_after']:.5f}, "
          f"smallest relative gain {min((b - a) / a for a, b in zip(l1, l1[1:])):.3e}")
    assert 2 <= len(l1) <= 51 and 1 <= fit["iters_run"] <= 50
    assert all(b >= a * (1 - 1e-6) for a, b in zip(l1, l1[1:]))
    assert fit["qerr_after"] < fit["qerr_before"] and l1[fit["iters_run"]] == max(l1)
    R = fit["R"].double().cpu()
    assert float((R.T @ R - torch.eye(64, dtype=torch.float64)).abs().max()) <= 1e-5
    assert torch.equal(rt.full_rotation(rt.compact_rotation(fit["R"], 64 // s), 64 // s), fit["R"])   # block-diagonal


# ---- 6. search and evaluation --------------------------------------------------------------------------------------------------------
def test_a_rotated_index_searches_the_rotated_codes(tmp_path, dev):
    """`GalleryIndex.fit_rotation().search(...)` is `hamming_topk` on `pack_sign(rotate_codes(...))` of both sides; the mean is
    subtracted before the rotation, text queries (mean_shift=False) are rotated unshifted; the mask plane is rebuilt from the rotated
    codes; the file round-trips; `concepts` needs blocks inside the sub-codes."""
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    V, lab = ir.clustered_case(1500, 64, seed=5)
    Q, _ = ir.clustered_case(40, 64, seed=6)
    g, q = _t(V, dev), _t(Q, dev)
    mean = g.mean(0)
    plain = GalleryIndex(rt.pack_sign(g - mean), 64, 4, labels=_t(lab, dev), mean=mean, mask=rt.confidence_mask(g - mean, 0.25), margin=0.25,
                         real=g - mean)
    index = plain.fit_rotation()
    assert index.rotation_blocks == 4 and index.keeps_concepts and plain.rotation is None
    fit = rt.fit_rotation(g - mean, 4)
    assert torch.equal(index.rotation, fit["R"]) and index.rotation_info["iters_run"] == fit["iters_run"]
    assert index.rotation_info["qerr_after"] < index.rotation_info["qerr_before"]
    rot = rt.rotate_codes(g - mean, fit["R"], 4)
    assert torch.equal(index.real, rot) and torch.equal(index.codes, rt.pack_sign(rot)) and torch.equal(index.mask, rt.confidence_mask(rot, 0.25))
    for shift in (True, False):
        qr = rt.rotate_codes(q - mean if shift else q, fit["R"], 4)
        idx, dist = rt.hamming_topk(rt.pack_sign(qr), rt.pack_sign(rot), 10)
        res = index.search(q, 10, mean_shift=shift)
        assert torch.equal(res["idx"], idx) and torch.equal(res["dist"], dist)
    own = index.search(plain.real[:50], 1, mean_shift=False)                # database rows as queries: each finds a row at distance 0
    assert bool((own["dist"] == 0).all())
    res = index.search(q, 5, concepts=[0, 2])
    idx, dist = rt.hamming_topk_masked(rt.pack_sign(rt.rotate_codes(q - mean, fit["R"], 4)), index.codes, rt.concept_mask(64, 4, [0, 2]).to(dev), 5)
    assert torch.equal(res["idx"], idx) and torch.equal(res["dist"], dist)
    full = plain.fit_rotation(blocks=1, iters=5)
    assert not full.keeps_concepts and full.rotation_info["blocks"] == 1
    with pytest.raises(ValueError, match="straddle"):
        full.search(q, 5, concepts=[0])
    assert tuple(full.search(q, 5)["idx"].shape) == (40, 5)
    with pytest.raises(ValueError, match="rotated already"):
        index.fit_rotation()
    path = str(tmp_path / "index.pth")
    index.save(path)
    back = GalleryIndex.load(path).to(dev)
    assert torch.equal(back.rotation, index.rotation) and back.rotation_blocks == 4 and back.rotation_info == index.rotation_info
    res2 = back.search(q, 10)
    assert torch.equal(res2["idx"], index.search(q, 10)["idx"])
    plain.save(path)
    assert not {"rotation", "rotation_blocks", "rotation_info"} & set(torch.load(path, map_location="cpu"))


COMMON = ["dataset=synthetic_cub200", "dataset.limit=96", "batch_size=32"]


def _search(tmp, logdir, name, common, **keys):
    """exp=search as main_v2.run starts it -> (the experiment, results.json)"""
    import main_v2
    from concepthash_amd import config as cfglib
    from experiments.search import SearchExperiment
    out = str(tmp / name)
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", ["logdir=" + logdir, "search_logdir=" + out] + common, cwd=str(tmp))
    for k, v in keys.items():
        cfg[k] = v
    ex = SearchExperiment(main_v2._run_config(cfg, "search", main_v2.SEARCH_KEYS))
    ex.main()
    return ex, json.load(open(os.path.join(out, "results.json")))


def test_the_search_and_the_validation_commands_under_a_rotation(tmp_path, dev, monkeypatch):
    import main_v2
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    monkeypatch.chdir(tmp_path)
    logdir = str(tmp_path / "run")
    common = COMMON + ["data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path))
    # exp=validation itq_eval=true
    ev = str(tmp_path / "ev")
    main_v2.main(["--config-name", "val.yaml", "logdir=" + logdir, "save_code=True", "itq_eval=true", "eval_logdir=" + ev] + common)
    hist = json.load(open(os.path.join(ev, "history.json")))
    outs = torch.load(os.path.join(ev, "outputs.pth"))
    te, db = outs["test"], outs["db"]
    gt, qt = db["codes"].to(dev, torch.float32), te["codes"].to(dev, torch.float32)
    ncontext = hist["itq_blocks"]
    for key in ("mAP_itq", "recalls_itq", "precisions_itq", "itq_blocks", "itq_iters_run", "quantisation_error", "quantisation_error_itq", "itq_gain"):
        assert key in hist, key
    fit = rt.fit_rotation(gt, hist["itq_blocks"])
    assert hist["itq_iters_run"] == fit["iters_run"]
    assert hist["quantisation_error"] == fit["qerr_before"] and hist["quantisation_error_itq"] == fit["qerr_after"]
    gr, qr = rt.rotate_codes(gt, fit["R"], ncontext), rt.rotate_codes(qt, fit["R"], ncontext)
    want = rt.evaluate(rt.pack_sign(qr), rt.pack_sign(gr), te["labels"].to(dev), db["labels"].to(dev), R=-1, ks=(1, 5, 10))   # val.yaml: R, PRs
    assert hist["mAP_itq"] == want["mAP"] and hist["recalls_itq"] == want["recalls"] and hist["precisions_itq"] == want["precisions"]
    assert hist["itq_gain"] == hist["mAP_itq"] - hist["mAP"]
    plain = rt.evaluate(rt.pack_sign(qt), rt.pack_sign(gt), te["labels"].to(dev), db["labels"].to(dev), R=-1, ks=(1, 5, 10))
    assert hist["mAP"] == plain["mAP"]                                       # the evaluator's own keys are what they were
    # exp=search rotate=itq: database images as queries
    ex, res = _search(tmp_path, logdir, "s1", common, rotate="itq", query="db", k=5)
    rot = res["rotation"]
    assert rot == dict(method="itq", blocks=ncontext, iters_run=fit["iters_run"], qerr_before=fit["qerr_before"], qerr_after=fit["qerr_after"],
                       keeps_concepts=True)
    assert res["index_status"] == "built: no index file" and len(res["queries"]) == 96 and res["ncontext"] == ncontext
    saved = GalleryIndex.load(os.path.join(logdir, "index_best.pth"))
    assert torch.equal(saved.rotation, fit["R"].cpu()) and saved.rotation_blocks == ncontext and torch.equal(saved.real, gr.cpu())
    assert torch.equal(saved.codes, rt.pack_sign(gr).cpu())
    idx, dist = rt.hamming_topk(rt.pack_sign(gr), rt.pack_sign(gr), 5)
    for i, e in enumerate(res["queries"]):
        assert e["hits"][0]["distance"] == 0 and [h["index"] for h in e["hits"]] == idx[i].tolist(), i
        assert [h["distance"] for h in e["hits"]] == dist[i].tolist()
    # the saved index is loaded by the same request, with concepts; one full rotation refuses them
    ex, res = _search(tmp_path, logdir, "s2", common, rotate="itq", concepts=[0], k=5)
    assert res["index_status"] == "loaded" and res["rotation"] == rot and res["concepts"] == [0]
    idx, _ = rt.hamming_topk_masked(rt.pack_sign(qr), rt.pack_sign(gr), rt.concept_mask(64, ncontext, [0]).to(dev), 5)
    assert [[h["index"] for h in e["hits"]] for e in res["queries"]] == idx.tolist()
    with pytest.raises(ValueError, match="straddle"):
        _search(tmp_path, logdir, "s3", common, rotate="itq", rotate_blocks=1, rotate_iters=3, concepts=[0], k=5)
    full = GalleryIndex.load(os.path.join(logdir, "index_best.pth"))
    assert full.rotation_blocks == 1 and not full.keeps_concepts
    # without rotate the rotated index is stale
    ex, res = _search(tmp_path, logdir, "s4", common, k=5)
    assert res["index_status"].startswith("built: stale index") and res["rotation"] is None
    assert GalleryIndex.load(os.path.join(logdir, "index_best.pth")).rotation is None
    idx, _ = rt.hamming_topk(rt.pack_sign(qt), rt.pack_sign(gt), 5)
    assert [[h["index"] for h in e["hits"]] for e in res["queries"]] == idx.tolist()


# the tiny run of tests/test_text_query_gpu.py (a local CLIP directory with a text tower, five class names): pytest instantiates the
# imported module-scoped fixture once more for this module, in a directory of its own
from test_text_query_gpu import run as text_run   # noqa: E402,F401


def test_text_queries_go_through_the_rotation(text_run, dev):
    """`exp=search query=classes rotate=itq`: the index is rebuilt with a rotation, and a class prompt's hits are those of the model's own
    folded centre row, rotated unshifted, against the rotated database -- its own neighbourhood in the rotated space."""
    import main_v2
    from concepthash_amd import config as cfglib, retrieval as rt
    from experiments.search import SearchExperiment
    from test_text_query_gpu import _compose

    def search(name, **keys):
        out = str(text_run["tmp"] / name)
        cfg = _compose("search.yaml", text_run["tmp"], "logdir=" + text_run["logdir"], "search_logdir=" + out)
        for k, v in keys.items():
            cfg[k] = v
        ex = SearchExperiment(main_v2._run_config(cfg, "search", main_v2.SEARCH_KEYS))
        ex.main()
        return ex, json.load(open(os.path.join(out, "results.json")))

    _, built = search("r0", query="classes", rotate="itq", k=7)
    assert built["index_status"].startswith("built: stale index") and built["rotation"]["method"] == "itq" and built["query_kind"] == "text"
    ex, res = search("r1", query="classes", rotate="itq", k=7)
    assert res["index_status"] == "loaded" and res["rotation"] == built["rotation"] and res["mean_shift"] is False
    index, model = ex.index.to(dev), ex.trainer.model
    codes = model.project_text(model.center)
    qr = rt.rotate_codes(codes.to(dev, torch.float32).contiguous(), index.rotation, index.rotation_blocks)
    idx, dist = rt.hamming_topk(rt.pack_sign(qr), index.codes, 7)
    assert len(res["queries"]) == 5
    for c, e in enumerate(res["queries"]):
        assert [h["index"] for h in e["hits"]] == idx[c].tolist() and [h["distance"] for h in e["hits"]] == dist[c].tolist(), c
    assert [[h["index"] for h in e["hits"]] for e in built["queries"]] == idx.tolist()
