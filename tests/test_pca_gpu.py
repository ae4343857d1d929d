"""GPU: the reduction ("reduction"; csrc/pca.hip) against the fp64 reference tests/pca_ref.py -- exact inputs
compared for equality at every segmentation, Gaussian inputs inside the derived bounds, the one projection chain (alone as in a batch,
and `rotate_codes` where t = s), the fit's captured variance, and the reduction in `GalleryIndex`, `exp=search reduce=...` and
`exp=validation reduce_eval=true`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import itq_ref as ir
import pca_ref as pr
from conftest import ROOT

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 63, 64, 65, 4097)
SEGS = (1, 64, None)
SHAPES = [(n, blocks) for n in (1, 24, 64, 256) for blocks in sorted({1, 4, n}) if n % blocks == 0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _moments(X, blocks, shift, seg, dev):
    from concepthash_amd import retrieval as rt
    total, gram = rt.pca_moments(_t(X, dev), blocks, _t(shift, dev), seg)
    return total.cpu().numpy(), gram.cpu().numpy()


def _project(X, mean, Ac, blocks, dev):
    from concepthash_amd import retrieval as rt
    return rt.project_codes(_t(X, dev), _t(mean, dev), _t(Ac, dev), blocks, compact=True).cpu().numpy()


@pytest.fixture(scope="module")
def grid():
    """the exact inputs, made once per width: (X [4097, n], shift [n]); fewer rows are its first rows"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = pr.grid_case(max(ROWS), n, seed=n)
        return made[n]
    return get


@pytest.fixture(scope="module")
def gauss():
    made = {}

    def get(n):
        if n not in made:
            X = pr.gaussian_case(max(ROWS), n, seed=100 + n)
            made[n] = X, X.astype(np.float64).mean(0).astype(np.float32)
        return made[n]
    return get


# ---- 1. moments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,blocks", SHAPES)
def test_exact_moments_equal_the_reference_at_every_segmentation(n, blocks, grid, dev):
    """Entries and shift are multiples of 1/16 in [-2, 2]: |y| <= 4, products are multiples of 2^-8 of at most 16, and a chain of at most
    4,096 of them stays below 2^24 units -- fp32 is exact, so sum and gram EQUAL the reference for every seg_rows, with and without a
    shift; two calls are bit-equal; gram is exactly symmetric inside a block."""
    Xall, shift = grid(n)
    s = n // blocks
    for rows in ROWS:
        X = Xall[:rows]
        for sh in (shift, None):
            total_ref, gram_ref = pr.moments(X, s, sh)
            for seg in SEGS:
                total, gram = _moments(X, blocks, sh, seg, dev)
                assert total.dtype == np.float64 and gram.dtype == np.float64 and total.shape == (n,) and gram.shape == (n, s)
                assert np.array_equal(total, total_ref), (rows, seg, sh is None)
                assert np.array_equal(gram, gram_ref), (rows, seg, sh is None, np.abs(gram - gram_ref).max())
        a, b = _moments(X, blocks, shift, 64, dev), _moments(X, blocks, shift, 64, dev)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


@pytest.mark.parametrize("n,blocks", SHAPES)
def test_gaussian_moments_stay_inside_the_derived_bounds(n, blocks, gauss, dev):
    """Rows N(3, 1), shifted by their fp32 mean and unshifted.  |gram - ref| <= (gamma_L + 2^-50) sum_i |y_a y_c| and |sum - ref| <=
    (gamma_L + 2^-50) sum_i |y|, L = min(rows, seg_rows), gamma_L = L u / (1 - L u), u = 2^-24; 2^-50: the fp64 combine of the
    segments (tests/pca_ref.py derives both).  Two calls give the same bits and gram is exactly symmetric inside a block."""
    Xall, mean = gauss(n)
    s = n // blocks
    worst = 0.0
    for rows in ROWS:
        X = Xall[:rows]
        for sh in (mean, None):
            total_ref, gram_ref = pr.moments(X, s, sh)
            for seg in SEGS:
                L = min(rows, pr.default_seg_rows(rows) if seg is None else seg)
                Bs, Bg = pr.moment_bounds(X, s, L, sh)
                total, gram = _moments(X, blocks, sh, seg, dev)
                worst = max(worst, float((np.abs(gram - gram_ref) / np.maximum(Bg, 1e-300)).max()), float((np.abs(total - total_ref) / np.maximum(Bs, 1e-300)).max()))
                assert (np.abs(gram - gram_ref) <= Bg).all(), (rows, seg, sh is None, float((np.abs(gram - gram_ref) - Bg).max()))
                assert (np.abs(total - total_ref) <= Bs).all(), (rows, seg, sh is None, float((np.abs(total - total_ref) - Bs).max()))
                G = gram.reshape(blocks, s, s)
                assert np.array_equal(G.view(np.uint64), np.ascontiguousarray(G.transpose(0, 2, 1)).view(np.uint64)), (rows, seg)
        a, b = _moments(X, blocks, mean, None, dev), _moments(X, blocks, mean, None, dev)
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    print(f"moments {n}/{blocks}: the largest error is {worst:.3f} of its bound")


def test_default_segment_rule_and_empty_input(dev):
    """the L the bounds use under seg_rows=None is the library's: its workspace is that of ceil(rows / default) segments"""
    from concepthash_amd import _lib, retrieval as rt
    lib = _lib.load()
    for rows in ROWS + (800, 100_000):
        seg = pr.default_seg_rows(rows)
        assert lib.ch_pca_moments_workspace(rows, 64, 16, 0, 1) == lib.ch_pca_moments_workspace(rows, 64, 16, seg, 1) == -(-rows // seg) * (64 + 64 * 16) * 4 + 16
    X = torch.zeros(0, 64, device=dev)
    total, gram = rt.pca_moments(X, 4)
    assert tuple(total.shape) == (64,) and tuple(gram.shape) == (64, 16) and float(gram.abs().max()) == 0
    assert tuple(rt.project_codes(X, None, torch.zeros(64, 8, device=dev), 4, compact=True).shape) == (0, 32)
    ws = torch.zeros(16, dtype=torch.int64, device=dev)
    out = torch.zeros(64, dtype=torch.float64, device=dev)
    x8 = torch.zeros(8, 64, device=dev)
    assert lib.ch_pca_moments(_lib.ptr(x8), 8, 64, 16, None, 0, _lib.ptr(out), None, _lib.ptr(ws), 8, _lib.stream_ptr()) == 2
    assert b"workspace too small" in lib.ch_last_error()


# ---- 2. projection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,blocks", SHAPES)
def test_the_projection_is_one_chain(n, blocks, grid, gauss, dev):
    """On the exact grid (A multiples of 1/16) out EQUALS the reference; on Gaussian input |out - ref| <= gamma_s sum_l |y_l| |A_lj|; row i
    of a batch equals the one-row call bit for bit; with t = s and no shift it is `rotate_codes` bit for bit; 65 rows of 64 outputs and
    fewer leave a ragged last workgroup of 256 lanes."""
    from concepthash_amd import retrieval as rt
    s = n // blocks
    Xg, shift = grid(n)
    Xn, mean = gauss(n)
    for t in sorted({1, (s + 1) // 2, s}):
        A = pr.grid_matrix(n, t, seed=n + t)
        for rows in ROWS:
            for sh in (shift, None):
                out = _project(Xg[:rows], sh, A, blocks, dev)
                assert out.dtype == np.float32 and out.shape == (rows, blocks * t)
                assert np.array_equal(out.astype(np.float64), pr.project(Xg[:rows], sh, A, s)), (t, rows, sh is None)
        R = ir.qr_rotation(n, s, np.random.default_rng(n + t))[:, :t].copy()
        for rows in (65, 4097):
            for sh in (mean, None):
                out = _project(Xn[:rows], sh, R, blocks, dev).astype(np.float64)
                excess = np.abs(out - pr.project(Xn[:rows], sh, R, s)) - pr.project_bound(Xn[:rows], sh, R, s)
                assert excess.max() <= 0, (t, rows, sh is None, excess.max())
        batch = _project(Xn[:65], mean, R, blocks, dev)
        for i in (0, 1, 63, 64):
            assert np.array_equal(_project(Xn[i:i + 1], mean, R, blocks, dev)[0].view(np.uint32), batch[i].view(np.uint32)), (t, i)
    R = ir.qr_rotation(n, s, np.random.default_rng(n))
    for rows in (1, 65, 4097):
        rot = rt.rotate_codes(_t(Xn[:rows], dev), _t(R, dev), blocks).cpu().numpy()
        assert np.array_equal(_project(Xn[:rows], None, R, blocks, dev).view(np.uint32), rot.view(np.uint32)), rows
    # the block-structured [n, bits] form is the compact one
    full = rt.full_projection(_t(R[:, :max(1, s // 2)].copy(), dev), blocks)
    assert torch.equal(rt.project_codes(_t(Xn[:65], dev), _t(mean, dev), full, blocks),
                       rt.project_codes(_t(Xn[:65], dev), _t(mean, dev), _t(R[:, :max(1, s // 2)].copy(), dev), blocks, compact=True))


# ---- 3. the fit ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """20 classes x 40 rows, sigma = 0.9, seed 0: (database [650, 64], its labels, queries [150, 64], their labels)"""
    return pr.planted_case(0.9, seed=0)


@pytest.mark.parametrize("method", ["pca-itq", "pca"])
def test_the_fit_captures_the_leading_variance(method, dev):
    """800 x 64, blocks 4, t = 8.  A has orthonormal columns per block to 1e-5 (in fp64), and per block tr(A_b^T C A_b) >= sum_{j <= t}
    lambda_j(C) - 2 t eps - 1e-5 tr(C), C the fp64 covariance of y = fl32(x - mean) and eps the Frobenius norm of the moment bounds over
    N - 1 (Weyl twice; a rotation keeps the trace: tests/pca_ref.py)."""
    from concepthash_amd import retrieval as rt
    g, _, q, _ = pr.planted_case(0.9, seed=2)
    X = np.concatenate([g, q])
    assert X.shape == (800, 64)
    fit = rt.fit_reduction(_t(X, dev), 32, 4, method=method)
    assert fit["bits"] == 32 and fit["blocks"] == 4 and fit["method"] == method and tuple(fit["A"].shape) == (64, 32)
    assert fit["A"].dtype == torch.float32 and fit["mean"].dtype == torch.float32 and (fit["iters_run"] > 0) == (method == "pca-itq")
    mean = fit["mean"].cpu().numpy()
    assert np.abs(mean.astype(np.float64) - X.astype(np.float64).mean(0)).max() <= 2.0 ** -22      # fp32(sum / N) of sums inside their bound
    A = rt.compact_projection(fit["A"], 4).cpu().numpy().astype(np.float64).reshape(4, 16, 8)
    total, gram = pr.moments(X, 16, mean)
    C = pr.covariance(total, gram, 800)
    eps = pr.fit_epsilon(X, mean, 16, min(800, pr.default_seg_rows(800)))
    for b in range(4):
        assert np.abs(A[b].T @ A[b] - np.eye(8)).max() <= 1e-5, b
        lam = np.linalg.eigvalsh(C[b])[::-1]
        got, want = np.trace(A[b].T @ C[b] @ A[b]), lam[:8].sum() - 2 * 8 * eps[b] - 1e-5 * np.trace(C[b])
        print(f"{method} block {b}: tr(A^T C A) = {got:.6f}, sum of the 8 largest eigenvalues {lam[:8].sum():.6f}, eps {eps[b]:.3e}, tr(C) {np.trace(C[b]):.4f}")
        assert got >= want, b
    ref = pr.fit(X, 32, 4, "pca")
    assert abs(fit["explained_share"] - ref["explained_share"]) <= 1e-5 and fit["explained_share"] > 0.9
    assert 0.0 < fit["qerr_after"] <= fit["qerr_pca"] + 1e-6
    if method == "pca":
        assert fit["qerr_after"] == fit["qerr_pca"]
        assert np.abs(rt.compact_projection(fit["A"], 4).cpu().numpy() - ref["A"]).max() <= 1e-4
    # a direction without variance is allowed and reported
    X2 = X.copy()
    X2[:, 5] = 1.25
    fit2 = rt.fit_reduction(_t(X2, dev), 64, 4, method="pca")
    assert abs(fit2["eigenvalues"][0][-1]) <= 1e-9 and abs(fit2["explained_share"] - 1.0) <= 1e-9


# ---- 4. the index --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indexes(planted, dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    g, gl, q, ql = planted
    gt = _t(g, dev)
    mean = gt.mean(0)
    plain = GalleryIndex(rt.pack_sign(gt - mean), 64, 4, labels=_t(gl, dev), mean=mean, mask=rt.confidence_mask(gt - mean, 0.25), margin=0.25,
                         real=gt - mean)
    return plain, plain.fit_reduction(32)


def test_a_database_row_finds_itself_at_distance_zero(indexes, dev):
    """A reduced index (64 -> 32, blocks 4) queried with its own database's 64-d real codes: the query goes through the chain the
    database went through, so its bits ARE the row's bits, and every list that contains the row has it at distance 0."""
    from concepthash_amd import retrieval as rt
    plain, index = indexes
    assert index.nbit == 32 and index.nbit_in == 64 and index.reduce_blocks == 4 and index.keeps_concepts and plain.reduce_A is None
    assert tuple(index.real.shape) == (650, 32) and tuple(index.codes.shape) == (650, 1) and tuple(index.mean.shape) == (64,)
    red = rt.project_codes(plain.real, index.reduce_mean, index.reduce_A, 4)
    assert torch.equal(index.real, red) and torch.equal(index.codes, rt.pack_sign(red)) and torch.equal(index.mask, rt.confidence_mask(red, 0.25))
    res = index.search(plain.real, 128, mean_shift=False)
    assert bool((res["dist"][:, 0] == 0).all())
    own = res["idx"] == torch.arange(650, device=dev)[:, None]
    assert int(own.any(1).sum()) >= 600 and bool((res["dist"][own] == 0).all())
    info = index.reduce_info
    assert info["method"] == "pca-itq" and info["bits"] == 32 and info["bits_in"] == 64 and info["blocks"] == 4
    assert set(info) == {"method", "bits", "bits_in", "blocks", "iters_run", "explained_share", "qerr_pca", "qerr_after"}
    with pytest.raises(ValueError, match="reduced already"):
        index.fit_reduction(16)


def test_the_lists_of_a_reduced_index(indexes, planted, tmp_path, dev):
    """The lists equal hamming_topk(pack_sign(project(q)), pack_sign(project(db))); concepts=[0, 2] ranks by the two 8-bit sub-codes;
    rank="cosine" runs on the reduced real plane; mean_shift=False still reduces; the file round-trips."""
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    plain, index = indexes
    q = _t(planted[2], dev)
    for shift in (True, False):
        qr = rt.project_codes((q - plain.mean) if shift else q, index.reduce_mean, index.reduce_A, 4)
        idx, dist = rt.hamming_topk(rt.pack_sign(qr), rt.pack_sign(index.real), 10)
        res = index.search(q, 10, mean_shift=shift)
        assert torch.equal(res["idx"], idx) and torch.equal(res["dist"], dist), shift
    qr = rt.project_codes(q - plain.mean, index.reduce_mean, index.reduce_A, 4)
    res = index.search(q, 5, concepts=[0, 2])
    idx, dist = rt.hamming_topk_masked(rt.pack_sign(qr), index.codes, rt.concept_mask(32, 4, [0, 2]).to(dev), 5)
    assert torch.equal(res["idx"], idx) and torch.equal(res["dist"], dist)
    assert tuple(res["concept_dist"].shape) == (150, 5, 4) and int(res["concept_dist"].max()) <= 8
    res = index.search(q, 7, rank="cosine")
    idx, dist = rt.dense_topk(rt.prepare_dense(qr, "cosine"), rt.prepare_dense(index.real, "cosine"), "cosine", 7)
    assert torch.equal(res["idx"], idx)
    tern = index.search(q, 5, rank="ternary", margin=0.25)
    assert tuple(tern["idx"].shape) == (150, 5)
    full = plain.fit_reduction(16, blocks=1, iters=5, method="pca")
    assert not full.keeps_concepts and full.nbit == 16 and full.reduce_info["iters_run"] == 0
    with pytest.raises(ValueError, match="straddle"):
        full.search(q, 5, concepts=[0])
    assert tuple(full.search(q, 5)["idx"].shape) == (150, 5)
    path = str(tmp_path / "index.pth")
    index.save(path)
    back = GalleryIndex.load(path, nbit=64).to(dev)
    assert torch.equal(back.reduce_A, index.reduce_A) and back.reduce_info == index.reduce_info
    assert torch.equal(back.search(q, 10)["idx"], index.search(q, 10)["idx"])


def test_the_planted_variance_is_recovered(planted, dev):
    """20 classes x 40 rows, 4 blocks of 16 dimensions: an 8-d latent of +-1 class centres + N(0, 0.9^2) beside 8 dimensions of
    N(0, 0.15^2), behind a random orthogonal 16 x 16 matrix, plus 0.7; 150 rows are queries.  At 32 bits mAP_reduce >= mAP_truncate +
    0.05: a third of the smallest gap of the construction, a guard against a fit that silently degenerates to truncation, not against
    rounding.  tests/pca_ref.py (`python tests/pca_ref.py`, fp64 numpy, this seed 0 and sigma 0.9) gives mAP@all
    full 64 bits 0.790, truncated 0.560, PCA 0.678, PCA-ITQ 0.792 (sigma 0.7: 0.938 / 0.753 / 0.842 / 0.952; 1.1: 0.603 / 0.393 /
    0.499 / 0.566)."""
    from concepthash_amd import retrieval as rt
    g, gl, q, ql = planted
    gt, qt, glt, qlt = _t(g, dev), _t(q, dev), _t(gl, dev), _t(ql, dev)
    mean = gt.mean(0)
    cols = torch.from_numpy(pr.truncated_columns(64, 32, 4)).to(dev)
    score = lambda a, b: rt.evaluate(rt.pack_sign(a.contiguous()), rt.pack_sign(b.contiguous()), qlt, glt, R=-1)["mAP"]
    full, cut = score(qt - mean, gt - mean), score((qt - mean)[:, cols], (gt - mean)[:, cols])
    got = {}
    for method in ("pca", "pca-itq"):
        fit = rt.fit_reduction(gt - mean, 32, 4, method=method)
        got[method] = score(rt.project_codes(qt - mean, fit["mean"], fit["A"], 4), rt.project_codes(gt - mean, fit["mean"], fit["A"], 4))
    print(f"planted: full {full:.4f}, truncated {cut:.4f}, pca {got['pca']:.4f}, pca-itq {got['pca-itq']:.4f}")
    assert got["pca-itq"] >= cut + 0.05
    ref = pr.planted_maps(0.9, seed=0)
    assert abs(full - ref["full"]) <= 1e-6 and abs(cut - ref["truncated"]) <= 1e-6       # the same sign codes, the same ranking rule


# ---- 5. the commands -----------------------------------------------------------------------------------------------------------------
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


def test_the_search_and_the_validation_commands_under_a_reduction(tmp_path, dev, monkeypatch):
    import main_v2
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    from experiments.reduce_eval import truncated_columns
    monkeypatch.chdir(tmp_path)
    logdir = str(tmp_path / "run")
    common = COMMON + ["data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path))
    # exp=validation reduce_eval=true
    ev = str(tmp_path / "ev")
    main_v2.main(["--config-name", "val.yaml", "logdir=" + logdir, "save_code=True", "reduce_eval=true", "reduce_bits=32", "eval_logdir=" + ev] + common)
    hist = json.load(open(os.path.join(ev, "history.json")))
    outs = torch.load(os.path.join(ev, "outputs.pth"))
    te, db = outs["test"], outs["db"]
    gt, qt = db["codes"].to(dev, torch.float32), te["codes"].to(dev, torch.float32)
    for key in ("mAP_reduce", "recalls_reduce", "precisions_reduce", "reduce_bits", "reduce_blocks", "reduce_method", "reduce_iters_run",
                "reduce_explained", "quantisation_error_reduce", "mAP_truncate", "reduce_gain"):
        assert key in hist, key
    ncontext = hist["reduce_blocks"]
    assert hist["reduce_bits"] == 32 and hist["reduce_method"] == "pca-itq" and ncontext == 4
    fit = rt.fit_reduction(gt, 32, ncontext)
    assert hist["reduce_iters_run"] == fit["iters_run"] and hist["reduce_explained"] == fit["explained_share"]
    assert hist["quantisation_error_reduce"] == fit["qerr_after"]
    gr, qr = rt.project_codes(gt, fit["mean"], fit["A"], ncontext), rt.project_codes(qt, fit["mean"], fit["A"], ncontext)
    tl, dl = te["labels"].to(dev), db["labels"].to(dev)
    want = rt.evaluate(rt.pack_sign(qr), rt.pack_sign(gr), tl, dl, R=-1, ks=(1, 5, 10))   # val.yaml: R, PRs
    assert hist["mAP_reduce"] == want["mAP"] and hist["recalls_reduce"] == want["recalls"] and hist["precisions_reduce"] == want["precisions"]
    cols = truncated_columns(64, 32, ncontext).to(dev)
    cut = rt.evaluate(rt.pack_sign(qt[:, cols].contiguous()), rt.pack_sign(gt[:, cols].contiguous()), tl, dl, R=-1, ks=(1, 5, 10))
    assert hist["mAP_truncate"] == cut["mAP"] and hist["reduce_gain"] == hist["mAP_reduce"] - hist["mAP_truncate"]
    plain = rt.evaluate(rt.pack_sign(qt), rt.pack_sign(gt), tl, dl, R=-1, ks=(1, 5, 10))
    assert hist["mAP"] == plain["mAP"]                                       # the evaluator's own keys are what they were
    # exp=search reduce=pca-itq reduce_bits=32: database images as queries
    ex, res = _search(tmp_path, logdir, "s1", common, reduce="pca-itq", reduce_bits=32, query="db", k=5)
    assert res["reduction"] == dict(method="pca-itq", bits=32, bits_in=64, blocks=ncontext, iters_run=fit["iters_run"],
                                    explained_share=fit["explained_share"], qerr_pca=fit["qerr_pca"], qerr_after=fit["qerr_after"], keeps_concepts=True)
    assert res["index_status"] == "built: no index file" and len(res["queries"]) == 96 and res["nbit"] == 32 and res["rotation"] is None
    saved = GalleryIndex.load(os.path.join(logdir, "index_best.pth"), nbit=64)
    assert torch.equal(saved.reduce_A, fit["A"].cpu()) and saved.reduce_blocks == ncontext and torch.equal(saved.real, gr.cpu())
    assert torch.equal(saved.codes, rt.pack_sign(gr).cpu())
    api = saved.to(dev).search(gt, 5, mean_shift=False)                     # the API on the saved index: the command's hits
    idx, dist = rt.hamming_topk(rt.pack_sign(gr), rt.pack_sign(gr), 5)
    assert torch.equal(api["idx"], idx) and torch.equal(api["dist"], dist)
    for i, e in enumerate(res["queries"]):
        assert e["hits"][0]["distance"] == 0 and [h["index"] for h in e["hits"]] == idx[i].tolist(), i
        assert [h["distance"] for h in e["hits"]] == dist[i].tolist()
    # the saved index is loaded by the same request, with concepts addressing the 8-bit sub-codes
    ex, res = _search(tmp_path, logdir, "s2", common, reduce="pca-itq", reduce_bits=32, concepts=[0], k=5)
    assert res["index_status"] == "loaded" and res["reduction"]["bits"] == 32 and res["concepts"] == [0]
    idx, _ = rt.hamming_topk_masked(rt.pack_sign(qr), rt.pack_sign(gr), rt.concept_mask(32, ncontext, [0]).to(dev), 5)
    assert [[h["index"] for h in e["hits"]] for e in res["queries"]] == idx.tolist()
    # another setting, and no reduction at all, find the index stale
    ex, res = _search(tmp_path, logdir, "s3", common, reduce="pca", reduce_bits=16, k=5)
    assert res["index_status"].startswith("built: stale index") and res["reduction"]["method"] == "pca" and res["nbit"] == 16
    ex, res = _search(tmp_path, logdir, "s4", common, k=5)
    assert res["index_status"].startswith("built: stale index") and res["reduction"] is None
    assert GalleryIndex.load(os.path.join(logdir, "index_best.pth")).reduce_A is None
    idx, _ = rt.hamming_topk(rt.pack_sign(qt), rt.pack_sign(gt), 5)
    assert [[h["index"] for h in e["hits"]] for e in res["queries"]] == idx.tolist()
