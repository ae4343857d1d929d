"""No GPU: the reduction ("reduction"; csrc/pca.hip) -- the host-side PCA against numpy, the fp64 reference's own
properties, every refusal (all of them in front of the first launch, so CPU tensors reach them), the C entries' declarations and
host-side refusals, the index file with and without the new planes, and the configuration keys."""
import os

import numpy as np
import pytest
import torch
import yaml

import pca_ref as pr
from conftest import ROOT


# ---- the host-side PCA ---------------------------------------------------------------------------------------------------------------
def _separated(blocks, s, seed):
    """symmetric matrices with eigenvalues s, s - 1, .. 1 (separated by 1) behind random orthogonal matrices"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(blocks):
        Q = np.linalg.qr(rng.standard_normal((s, s)))[0]
        C = Q @ np.diag(np.arange(s, 0, -1.0)) @ Q.T
        out.append((C + C.T) / 2)
    return np.stack(out)


@pytest.mark.parametrize("blocks,s,t", [(1, 16, 16), (4, 16, 8), (3, 8, 1), (2, 64, 20), (5, 1, 1)])
def test_pca_components_is_numpys_eigh_under_the_sign_convention(blocks, s, t):
    from concepthash_amd import retrieval as rt
    C = _separated(blocks, s, seed=blocks + s + t)
    P, lam = rt.pca_components(torch.from_numpy(C), t)
    P_ref, lam_ref = pr.components(C, t)
    assert P.dtype == torch.float64 and tuple(P.shape) == (blocks, s, t) and tuple(lam.shape) == (blocks, s)
    assert np.abs(P.numpy() - P_ref).max() <= 1e-10 and np.abs(lam.numpy() - lam_ref).max() <= 1e-10
    assert bool((lam[:, :-1] >= lam[:, 1:]).all())                                      # descending
    lead = P.abs().argmax(1)
    assert bool((P.gather(1, lead[:, None, :]) > 0).all())                              # the largest entry of a component is positive


def test_the_sign_convention_takes_the_lowest_index_among_equals():
    from concepthash_amd import retrieval as rt
    # C = [[2, -1], [-1, 2]]: the leading eigenvector is (1, -1) / sqrt(2) up to sign -- two entries of equal magnitude; the first is made positive
    P, lam = rt.pca_components(torch.tensor([[[2.0, -1.0], [-1.0, 2.0]]], dtype=torch.float64), 2)
    assert np.allclose(lam.numpy(), [[3.0, 1.0]]) and P[0, 0, 0] > 0 and P[0, 1, 0] < 0 and P[0, 0, 1] > 0
    assert np.allclose(pr.signed(np.array([[-1.0], [1.0]])), [[1.0], [-1.0]])
    for bad, err in ((torch.zeros(2, 3, 3), TypeError), (torch.zeros(3, 3, dtype=torch.float64), ValueError),
                     (torch.zeros(1, 3, 4, dtype=torch.float64), ValueError), (torch.full((1, 2, 2), float("nan"), dtype=torch.float64), ValueError)):
        with pytest.raises(err):
            rt.pca_components(bad, 1)
    for t in (0, 4, 1.5, True):
        with pytest.raises(ValueError, match="t must be an int"):
            rt.pca_components(torch.eye(3, dtype=torch.float64)[None], t)


@pytest.mark.parametrize("method", ["pca", "pca-itq"])
def test_the_reference_fit_has_orthonormal_columns_per_block(method):
    g, _, _, _ = pr.planted_case(0.9, seed=1)
    f = pr.fit(g, 32, 4, method, iters=10)
    A = f["A"].astype(np.float64).reshape(4, 16, 8)
    for b in range(4):
        assert np.abs(A[b].T @ A[b] - np.eye(8)).max() <= 1e-6, b
    assert 0.5 < f["explained_share"] <= 1.0 and (f["iters_run"] > 0) == (method == "pca-itq")
    # the planted noise dimensions are what is dropped: the kept share is nearly all of the variance
    assert f["explained_share"] > 0.95
    # a direction without variance is allowed and shows as a zero eigenvalue
    g2 = g.copy()
    g2[:, 5] = 1.25
    f2 = pr.fit(g2, 64, 4, "pca")
    assert abs(f2["eigenvalues"][0, -1]) <= 1e-12 and abs(f2["explained_share"] - 1.0) <= 1e-12


def test_compact_and_full_projection():
    from concepthash_amd import retrieval as rt
    blocks = [torch.randn(4, 2), torch.randn(4, 2), torch.randn(4, 2)]
    F = torch.block_diag(*blocks)
    C = rt.compact_projection(F, 3)
    assert tuple(F.shape) == (12, 6) and tuple(C.shape) == (12, 2) and torch.equal(C[4:8], blocks[1]) and torch.equal(rt.full_projection(C, 3), F)
    F[0, 5] = 1.0
    with pytest.raises(ValueError, match="not block-structured"):
        rt.compact_projection(F, 3)
    with pytest.raises(ValueError, match="multiple of blocks"):
        rt.compact_projection(torch.zeros(12, 5), 3)
    assert pr.truncated_columns(64, 32, 4).tolist() == [b * 16 + j for b in range(4) for j in range(8)]


# ---- refusals, all in front of the first launch --------------------------------------------------------------------------------------
def test_every_refusal_is_raised_on_cpu_tensors():
    from concepthash_amd import retrieval as rt
    X = torch.randn(10, 64)
    for bits in (3, 65, 30, 0, 2.5, True):                      # not in [blocks, n], or no multiple of blocks
        with pytest.raises(ValueError, match="bits must be an int in"):
            rt.fit_reduction(X, bits, 4)
    with pytest.raises(ValueError, match="does not divide"):
        rt.fit_reduction(X, 32, 5)
    with pytest.raises(ValueError, match="at least 2 rows"):
        rt.fit_reduction(X[:1], 32, 4)
    with pytest.raises(ValueError, match="at least 2 rows"):
        rt.fit_reduction(X[:0], 32, 4)
    bad = X.clone()
    bad[3, 7] = float("inf")
    for fn in (lambda: rt.fit_reduction(bad, 32, 4), lambda: rt.pca_moments(bad, 4), lambda: rt.project_codes(bad, None, torch.zeros(64, 32), 4)):
        with pytest.raises(ValueError, match="NaN or infinite"):
            fn()
    with pytest.raises(ValueError, match="method must be one of"):
        rt.fit_reduction(X, 32, 4, method="itq")
    with pytest.raises(ValueError, match="iters must be an int"):
        rt.fit_reduction(X, 32, 4, iters=-1)
    with pytest.raises(TypeError, match="float32"):
        rt.fit_reduction(X.double(), 32, 4)
    with pytest.raises(ValueError, match="takes 1 .. 256"):
        rt.pca_moments(torch.zeros(4, 257), 1)
    with pytest.raises(ValueError, match="2-D"):
        rt.pca_moments(torch.zeros(4), 1)
    for seg in (0, 4097, -1):
        with pytest.raises(ValueError, match="seg_rows must be in"):
            rt.pca_moments(X, 4, seg_rows=seg)
    with pytest.raises(ValueError, match=r"shift must be a float32 tensor \[64\]"):
        rt.pca_moments(X, 4, shift=torch.zeros(32))
    with pytest.raises(ValueError, match="shift holds NaN"):
        rt.pca_moments(X, 4, shift=torch.full((64,), float("nan")))
    with pytest.raises(ValueError, match=r"mean must be a float32 tensor \[64\]"):
        rt.project_codes(X, torch.zeros(64, dtype=torch.float64), torch.zeros(64, 32), 4)
    with pytest.raises(ValueError, match="A must be a float32 tensor with 64 rows"):
        rt.project_codes(X, None, torch.zeros(32, 32), 4)
    with pytest.raises(ValueError, match="not block-structured"):
        rt.project_codes(X, None, torch.ones(64, 32), 4)
    with pytest.raises(ValueError, match="projects to 1 .. 16 columns"):
        rt.project_codes(X, None, torch.zeros(64, 17), 4, compact=True)
    # behind the checks: no CPU fallback
    for fn in (lambda: rt.fit_reduction(X, 32, 4), lambda: rt.pca_moments(X, 4), lambda: rt.project_codes(X, None, torch.zeros(64, 32), 4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    from concepthash_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "concepthash_hip.h")).read()
    for name in ("ch_pca_moments_workspace", "ch_pca_moments", "ch_pca_project"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert "#define CH_ABI_VERSION 3" in header and lib.ch_abi_version() == 3
    assert "pca.hip" in build.SOURCES and build.EXTRA_FLAGS["pca.hip"] == ["-ffp-contract=off"]
    # the host-side refusals (status 2, the house messages); rows == 0 is no error and launches nothing
    m = lambda rows, n, s, seg: lib.ch_pca_moments(None, rows, n, s, None, seg, None, None, None, 0, None)
    assert m(5, 300, 4, 0) == 2 and b"pca_moments: n must be in [1, 256]" in lib.ch_last_error()
    assert m(5, 64, 5, 0) == 2 and b"block must be >= 1 and divide n" in lib.ch_last_error()
    assert m(-5, 64, 16, 0) == 2 and b"negative rows" in lib.ch_last_error()
    assert m(5, 64, 16, 0) == 2 and b"null pointer" in lib.ch_last_error()
    assert m(5, 64, 16, 4097) == 2 and b"seg_rows" in lib.ch_last_error()
    assert m(0, 64, 16, 0) == 0
    p = lambda rows, n, s, t: lib.ch_pca_project(None, rows, n, s, None, None, t, None, None)
    assert p(5, 0, 1, 1) == 2 and b"pca_project: n must be in [1, 256]" in lib.ch_last_error()
    assert p(5, 64, 16, 17) == 2 and b"t must be in [1, block]" in lib.ch_last_error()
    assert p(5, 64, 16, 0) == 2 and b"t must be in [1, block]" in lib.ch_last_error()
    assert p(5, 64, 16, 8) == 2 and b"null pointer" in lib.ch_last_error()
    assert p(0, 64, 16, 8) == 0
    # the workspace: per segment n fp32 sums and, with the Gram, the n x s fp32 partial; 1M rows -> 977 segments of 1,024 rows
    assert lib.ch_pca_moments_workspace(1_000_000, 64, 16, 0, 1) == 977 * (64 + 64 * 16) * 4 + 16
    assert lib.ch_pca_moments_workspace(1_000_000, 64, 16, 0, 0) == 977 * 64 * 4 + 16
    assert lib.ch_pca_moments_workspace(513, 64, 16, 256, 1) == 3 * (64 + 64 * 16) * 4 + 16
    for rows in (1, 64, 65, 800, 4097, 1_000_000, 10_000_000):
        seg = pr.default_seg_rows(rows)
        assert lib.ch_pca_moments_workspace(rows, 8, 8, 0, 0) == -(-rows // seg) * 8 * 4 + 16, rows


# ---- the index -----------------------------------------------------------------------------------------------------------------------
def _index(nbit=64, **k):
    from concepthash_amd.search import GalleryIndex
    return GalleryIndex(torch.zeros(6, 1, dtype=torch.int64), nbit, 4, **k)


def _reduction(blocks=4, bits=32, n=64):
    from concepthash_amd import retrieval as rt
    return dict(reduce_mean=torch.randn(n), reduce_A=rt.full_projection(torch.randn(n, bits // blocks), blocks), reduce_blocks=blocks,
                reduce_info={"method": "pca-itq", "bits": bits, "bits_in": n, "blocks": blocks})


def test_index_refusals_and_nbit_in():
    from concepthash_amd.search import StaleIndexError
    with pytest.raises(ValueError, match="needs the index's real plane"):
        _index().fit_reduction(32)
    with pytest.raises(ValueError, match="rotated already"):
        _index(rotation=torch.eye(64), rotation_blocks=4, real=torch.zeros(6, 64)).fit_reduction(32)
    red = _index(32, real=torch.zeros(6, 32), **_reduction())
    with pytest.raises(ValueError, match="reduced already"):
        red.fit_reduction(16)
    for bits in (3, 65, 30):
        with pytest.raises(ValueError, match="bits must be an int in"):
            _index(real=torch.zeros(6, 64)).fit_reduction(bits)
    with pytest.raises(ValueError, match="does not divide"):
        _index(real=torch.zeros(6, 64)).fit_reduction(32, blocks=5)
    with pytest.raises(ValueError, match="not a multiple of ncontext"):
        _index(real=torch.zeros(6, 64)).fit_reduction(2, blocks=1)
    with pytest.raises(ValueError, match="method must be one of"):
        _index(real=torch.zeros(6, 64)).fit_reduction(32, method="svd")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _index(real=torch.randn(6, 64)).fit_reduction(32)
    with pytest.raises(ValueError, match=r"reduce_A must be a float32 matrix \[nbit_in, 32\]"):
        _index(32, **dict(_reduction(), reduce_A=torch.zeros(64, 16)))
    with pytest.raises(ValueError, match="reduce_mean must be the float32 centre"):
        _index(32, **dict(_reduction(), reduce_mean=torch.zeros(32)))
    with pytest.raises(ValueError, match="not block-structured"):
        _index(32, **dict(_reduction(), reduce_A=torch.ones(64, 32)))
    with pytest.raises(ValueError, match="without reduce_A"):
        _index(reduce_blocks=4)
    assert _index().nbit_in == 64 and red.nbit_in == 64 and red.nbit == 32 and red.keeps_concepts
    # the zero-mean plane is as wide as the queries; check() compares the model's width with nbit_in
    assert _index(32, mean=torch.zeros(64), **_reduction()).mean.shape[0] == 64
    with pytest.raises(ValueError, match=r"mean must be \[64\]"):
        _index(32, mean=torch.zeros(32), **_reduction())
    red.check(nbit=64)
    with pytest.raises(StaleIndexError, match="holds 64-bit codes but the model produces 32-bit"):
        red.check(nbit=32)
    with pytest.raises(ValueError, match=r"query codes must be \[Qn, 64\]"):
        red.search(torch.zeros(2, 32), 3)
    full = _index(32, **_reduction(blocks=1))
    assert not full.keeps_concepts
    with pytest.raises(ValueError, match="straddle"):
        full.search(torch.zeros(2, 64), 3, concepts=[0])


def test_the_index_file_carries_the_new_planes_and_an_old_file_still_loads(tmp_path):
    from concepthash_amd.search import FORMAT, GalleryIndex
    path = str(tmp_path / "a.pth")
    red = _index(32, real=torch.randn(6, 32), mean=torch.randn(64), **_reduction())
    red.save(path)
    d = torch.load(path)
    assert {"reduce_mean", "reduce_A", "reduce_blocks", "reduce_info"} <= set(d) and d["nbit"] == 32
    back = GalleryIndex.load(path, nbit=64)
    assert torch.equal(back.reduce_A, red.reduce_A) and torch.equal(back.reduce_mean, red.reduce_mean) and back.reduce_blocks == 4
    assert back.reduce_info == red.reduce_info and back.nbit == 32 and back.nbit_in == 64 and torch.equal(back.mean, red.mean)
    moved = back.to("cpu")
    assert torch.equal(moved.reduce_A, red.reduce_A) and moved.reduce_blocks == 4 and moved.reduce_info == red.reduce_info
    # an index without a reduction is the file it has always been, and a file written before the keys existed loads as before
    plain = _index(labels=torch.arange(6))
    plain.save(path)
    assert sorted(torch.load(path)) == sorted(["format", "codes", "nbit", "ncontext", "labels", "paths", "data_root", "mean", "transform", "fingerprint"])
    torch.save({"format": FORMAT, "codes": plain.codes, "nbit": 64, "ncontext": 4, "labels": plain.labels, "paths": None, "data_root": None,
                "mean": None, "transform": {}, "fingerprint": {}}, path)
    old = GalleryIndex.load(path, nbit=64)
    assert old.reduce_A is None and old.reduce_mean is None and old.reduce_blocks is None and old.reduce_info is None and old.nbit_in == 64


# ---- configuration -------------------------------------------------------------------------------------------------------------------
def _run_dir(tmp_path):
    run = tmp_path / "run"
    run.mkdir(exist_ok=True)
    (run / "config.yaml").write_text(yaml.safe_dump({
        "seed": 7, "batch_size": 32, "exp": "hashing", "trainer": {"_target_": "trainers.coop.COOPTrainer"},
        "model": {"_target_": "models.arch.coop.LGHWithFixedPrompt", "nbit": 64, "ncontext": 4, "backbone": {"name": "synthetic/clip-vit-small-patch16"}}}))
    return str(run)


def _config(tmp_path, name, keys, *overrides):
    import main_v2
    from concepthash_amd import config as cfglib
    out = "search_logdir=" if name == "search.yaml" else "eval_logdir="
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), name,
                         ["logdir=" + _run_dir(tmp_path), "dataset=synthetic_cub200", "data_dir=" + str(tmp_path), out + str(tmp_path / "o")]
                         + list(overrides), cwd=str(tmp_path))
    return main_v2._run_config(cfg, "search" if name == "search.yaml" else "validation", keys)


def test_the_new_keys_compose_and_default_to_no_reduction(tmp_path):
    import main_v2
    from experiments.reduce_eval import check_reduce_settings, truncated_columns
    from experiments.search import reduction_request
    assert {"reduce", "reduce_bits", "reduce_blocks", "reduce_iters"} <= set(main_v2.SEARCH_KEYS)
    assert {"reduce_eval", "reduce_bits", "reduce_method", "reduce_blocks", "reduce_iters"} <= set(main_v2.LOOP_KEYS)
    cfg = _config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS)
    assert cfg.reduce is None and cfg.reduce_bits is None and cfg.reduce_blocks is None and cfg.reduce_iters is None
    assert reduction_request(cfg) is None
    cfg = _config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, "reduce=pca-itq", "reduce_bits=32")
    assert reduction_request(cfg) == {"method": "pca-itq", "bits": 32, "blocks": 4, "iters": 50}          # one block per concept
    cfg = _config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, "reduce=pca", "reduce_bits=16", "reduce_blocks=1", "reduce_iters=7")
    assert reduction_request(cfg) == {"method": "pca", "bits": 16, "blocks": 1, "iters": 7}
    for overrides, word in ((["reduce=pca-itq", "reduce_bits=32", "rotate=itq"], "together with rotate"),
                            (["reduce=pca-itq"], "needs reduce_bits"), (["reduce=svd", "reduce_bits=32"], "reduce must be one of"),
                            (["reduce_bits=32"], "without reduce="), (["reduce=pca", "reduce_bits=30"], "reduce_bits must be an int"),
                            (["reduce=pca", "reduce_bits=128"], "reduce_bits must be an int"),
                            (["reduce=pca", "reduce_bits=32", "reduce_blocks=5"], "divides nbit = 64"),
                            (["reduce=pca", "reduce_bits=2", "reduce_blocks=1"], "ncontext = 4"),
                            (["reduce=pca", "reduce_bits=32", "reduce_iters=0"], "reduce_iters")):
        with pytest.raises(ValueError, match=word):
            reduction_request(_config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, *overrides))
    val = _config(tmp_path, "val.yaml", main_v2.EVAL_KEYS)
    assert val.reduce_eval is False and val.reduce_bits is None and val.reduce_method is None and val.reduce_blocks is None
    val = _config(tmp_path, "val.yaml", main_v2.EVAL_KEYS, "reduce_eval=true", "reduce_bits=32", "reduce_blocks=2")
    assert val.reduce_eval is True
    assert check_reduce_settings(val.reduce_bits, val.reduce_method, val.reduce_blocks, val.reduce_iters, val.model.ncontext) == (32, "pca-itq", 2, 50)
    assert check_reduce_settings(16, "pca", None, 9, 4) == (16, "pca", 4, 9)
    for args in ((None, None, None, None), (0, None, None, None), (2.5, None, None, None), (32, "svd", None, None), (32, None, 0, None),
                 (32, None, True, None), (32, None, None, 0)):
        with pytest.raises(ValueError, match="reduce_eval: "):
            check_reduce_settings(*args, 4)
    assert truncated_columns(64, 32, 4).tolist() == pr.truncated_columns(64, 32, 4).tolist()


def test_the_search_experiment_refuses_reduce_with_rotate_before_anything_is_loaded(tmp_path):
    import main_v2
    from experiments.search import SearchExperiment
    with pytest.raises(ValueError, match="together with rotate"):
        SearchExperiment(_config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, "reduce=pca-itq", "reduce_bits=32", "rotate=itq"))
    with pytest.raises(ValueError, match="needs reduce_bits"):
        SearchExperiment(_config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, "reduce=pca"))


def test_the_evaluator_refuses_what_it_cannot_reduce(monkeypatch):
    import utils.hashing
    from concepthash_amd.distributed import RowShard
    from experiments.reduce_eval import reduced_pair
    with pytest.raises(ValueError, match=r"reduce_eval: .*does not divide.*evaluated code width is 32"):
        reduced_pair(torch.zeros(4, 32), torch.zeros(2, 32), 15, 5, 50, "pca-itq")
    with pytest.raises(ValueError, match=r"reduce_eval: bits must be an int in.*evaluated code width is 16"):
        reduced_pair(torch.zeros(4, 16), torch.zeros(2, 16), 32, 4, 50, "pca-itq")
    shard = RowShard.__new__(RowShard)
    with pytest.raises(NotImplementedError, match="one process"):
        utils.hashing._single_process("hamming after reduce_eval", shard, None)
    monkeypatch.setattr(utils.hashing, "_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="one process"):
        utils.hashing._single_process("hamming after reduce_eval", torch.zeros(1, 1))


def test_main_v2_runs_the_reduce_evaluator_only_when_asked(tmp_path, monkeypatch):
    import main_v2
    import experiments.itq_eval as ie
    import experiments.reduce_eval as re_
    made = []
    for mod, name in ((re_, "ReduceEvaluation"), (ie, "ItqEvaluation")):
        cls = type(name, (), {"__init__": lambda self, cfg, n=name: made.append(n), "main": lambda self: None})
        monkeypatch.setattr(mod, name, cls)
    from concepthash_amd import config as cfglib

    def run(*overrides):
        cfg = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml",
                             ["logdir=" + _run_dir(tmp_path), "dataset=synthetic_cub200", "data_dir=" + str(tmp_path)] + list(overrides), cwd=str(tmp_path))
        main_v2.run(cfg)
    run("reduce_eval=true", "reduce_bits=32")
    run("itq_eval=true")
    assert made == ["ReduceEvaluation", "ItqEvaluation"]
