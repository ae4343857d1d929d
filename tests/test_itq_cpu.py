"""CPU: the host side of the learned rotation ("learned rotation") -- the fp64 reference tests/itq_ref.py against
its own definition, every argument refusal (all raised before anything touches a GPU: there is none here), the configuration keys, the
index file of an unrotated index, and the binding of the three C entries."""
import os

import numpy as np
import pytest
import torch
import yaml

import itq_ref as ir
from conftest import ROOT


# ---- the reference against itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [16, 64])
def test_the_reference_fit_never_loses_l1_and_stays_orthogonal(s):
    V, _ = ir.clustered_case(1200, 64, seed=3)
    V = V.astype(np.float64)
    R = ir.identity(64, s)
    l1s = []
    for _ in range(50):
        M, l1, cos, qerr, z = ir.step(V, R)
        l1s.append(l1)
        assert abs(qerr - (1 - cos / 1200)) < 1e-15
        # |B - V R|^2 = |V|^2 - 2 L1 + G n: the objective the fit maximises
        assert abs(((ir.sign(z) - z) ** 2).sum() - ((V * V).sum() - 2 * l1 + 1200 * 64)) < 1e-6
        R = ir.procrustes(M)
        F = ir.full(R)
        assert np.abs(F.T @ F - np.eye(64)).max() <= 1e-12
        off = F.copy()
        for b in range(64 // s):
            # the update is the Procrustes solution: tr(R_b M_b) = the sum of M_b's singular values, the most an orthogonal matrix gives
            Mb = M[b * s:(b + 1) * s]
            assert abs(np.trace(R[b * s:(b + 1) * s] @ Mb) - np.linalg.svd(Mb, compute_uv=False).sum()) <= 1e-9 * np.abs(Mb).sum()
            off[b * s:(b + 1) * s, b * s:(b + 1) * s] = 0
        assert not off.any()
    assert all(b >= a for a, b in zip(l1s, l1s[1:])) and l1s[-1] > 1.05 * l1s[0]


def test_the_reference_recovers_the_planted_rotation():
    V = ir.planted_case(4096, 64, 16, seed=4096)
    fit = ir.fit(V, 16)
    assert 0.15 < fit["qerr_before"] < 0.16 and 0.038 < fit["qerr_after"] < 0.040 and fit["iters_run"] <= 3
    z = ir.chain(V, fit["R"])
    assert np.abs(z).min() >= 0.4
    Q = np.tile(ir.givens_rotation(16), (4, 1))
    assert np.abs(fit["R"] - Q).max() < 0.02                                # V Q0 = X: the fit finds Q0 up to what a*B0 statistics leave


def test_sign_rule_and_zero_rows():
    assert ir.sign(np.array([0.0, -0.0, 1e-300, -1e-300])).tolist() == [-1, -1, 1, -1]
    M, l1, cos, qerr, _ = ir.step(np.zeros((3, 8)), ir.identity(8, 4))
    assert l1 == 0 and cos == 0 and qerr == 1.0
    V, R = ir.exact_case(130, 16, 4)
    M, _, _, _, z = ir.step(V, R)
    assert (z == 0).any() and np.array_equal(ir.chain(V, R).astype(np.float32).astype(np.float64), z)


# ---- argument refusals of the Python entries -----------------------------------------------------------------------------------------
def test_retrieval_entries_refuse_bad_arguments_before_any_launch():
    from concepthash_amd import retrieval as rt
    V, R = torch.randn(10, 8), torch.eye(8)
    for fn in (lambda c, r, b: rt.itq_step(c, r, b), rt.rotate_codes):
        with pytest.raises(TypeError, match="codes must be a float32 tensor"):
            fn(V.double(), R, 2)
        with pytest.raises(TypeError, match="R must be a float32 tensor"):
            fn(V, R.double(), 2)
        with pytest.raises(ValueError, match="2-D"):
            fn(V[0], R, 2)
        with pytest.raises(ValueError, match=r"1 \.\. 256"):
            fn(torch.randn(2, 300), torch.eye(300), 2)
        with pytest.raises(ValueError, match="does not divide"):
            fn(V, R, 3)
        with pytest.raises(ValueError, match="blocks must be an int"):
            fn(V, R, 2.0)
        with pytest.raises(ValueError, match=r"R must be \[8, 8\].*or \[8, 4\]"):
            fn(V, torch.eye(4), 2)
        with pytest.raises(ValueError, match="not block-diagonal"):
            fn(V, torch.ones(8, 8), 2)
        with pytest.raises(ValueError, match="NaN or infinite"):
            fn(torch.full((2, 8), float("nan")), R, 2)
        with pytest.raises(ValueError, match="NaN or infinite"):
            fn(V, R * float("inf"), 1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(V, R, 2)
    for bad in (0, 5000, -1):
        with pytest.raises(ValueError, match="seg_rows"):
            rt.itq_step(V, R, 2, seg_rows=bad)
    with pytest.raises(ValueError, match="does not divide"):
        rt.fit_rotation(V, 3)
    with pytest.raises(ValueError, match="NaN or infinite"):
        rt.fit_rotation(V * float("inf"), 2)
    with pytest.raises(ValueError, match="iters"):
        rt.fit_rotation(V, 2, iters=-1)
    with pytest.raises(ValueError, match="tol"):
        rt.fit_rotation(V, 2, tol=-1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rt.fit_rotation(V, 2)
    # the compact form and back
    F = torch.block_diag(torch.randn(4, 4), torch.randn(4, 4))
    C = rt.compact_rotation(F, 2)
    assert tuple(C.shape) == (8, 4) and torch.equal(C[4:], F[4:, 4:]) and torch.equal(rt.full_rotation(C, 2), F)
    # the update: W U^T of M = U S W^T, compact
    M = torch.randn(8, 4, dtype=torch.float64)
    assert np.allclose(rt.procrustes_update(M, 2).numpy(), ir.procrustes(M.numpy()), atol=1e-12)


def _index(**k):
    from concepthash_amd.search import GalleryIndex
    return GalleryIndex(torch.zeros(6, 1, dtype=torch.int64), 64, 4, **k)


def test_index_refusals_and_the_unrotated_file(tmp_path):
    from concepthash_amd.search import FORMAT, GalleryIndex
    with pytest.raises(ValueError, match="needs the index's real plane"):
        _index().fit_rotation()
    with pytest.raises(ValueError, match="does not divide"):
        _index(real=torch.zeros(6, 64)).fit_rotation(blocks=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _index(real=torch.randn(6, 64)).fit_rotation()
    with pytest.raises(ValueError, match=r"rotation must be the float32 matrix \[64, 64\]"):
        _index(rotation=torch.eye(32), rotation_blocks=4)
    with pytest.raises(ValueError, match="does not divide"):
        _index(rotation=torch.eye(64), rotation_blocks=5)
    with pytest.raises(ValueError, match="without a rotation"):
        _index(rotation_blocks=4)
    full = _index(rotation=torch.eye(64), rotation_blocks=1, rotation_info={"method": "itq"})
    assert not full.keeps_concepts and _index(rotation=torch.eye(64), rotation_blocks=8).keeps_concepts and _index().keeps_concepts
    with pytest.raises(ValueError, match="straddle"):
        full.search(torch.zeros(2, 64), 3, concepts=[0])
    with pytest.raises(ValueError, match="rotated already"):
        _index(rotation=torch.eye(64), rotation_blocks=4, real=torch.zeros(6, 64)).fit_rotation()
    # an index without a rotation is the file it has always been: the same keys, the same bytes as the dict written by hand
    (tmp_path / "hand").mkdir()
    path, by_hand = str(tmp_path / "a.pth"), str(tmp_path / "hand" / f"a.pth.tmp{os.getpid()}")   # the archive records the name it was written under
    idx = _index(labels=torch.arange(6))
    idx.save(path)
    d = torch.load(path)
    assert sorted(d) == sorted(["format", "codes", "nbit", "ncontext", "labels", "paths", "data_root", "mean", "transform", "fingerprint"])
    torch.save({"format": FORMAT, "codes": idx.codes, "nbit": 64, "ncontext": 4, "labels": idx.labels, "paths": None, "data_root": None,
                "mean": None, "transform": {}, "fingerprint": {}}, by_hand)
    assert open(path, "rb").read() == open(by_hand, "rb").read()
    back = GalleryIndex.load(path)
    assert back.rotation is None and back.rotation_blocks is None and back.rotation_info is None
    # and a rotated one round-trips
    full.save(path)
    back = GalleryIndex.load(path)
    assert torch.equal(back.rotation, torch.eye(64)) and back.rotation_blocks == 1 and back.rotation_info == {"method": "itq"}


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


def test_the_new_keys_compose_and_default_to_no_rotation(tmp_path):
    import main_v2
    from experiments.itq_eval import check_itq_settings
    from experiments.search import rotation_request
    assert {"rotate", "rotate_blocks", "rotate_iters"} <= set(main_v2.SEARCH_KEYS) and {"itq_eval", "itq_blocks", "itq_iters"} <= set(main_v2.LOOP_KEYS)
    cfg = _config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS)
    assert cfg.rotate is None and cfg.rotate_blocks is None and cfg.rotate_iters == 50 and rotation_request(cfg) is None
    cfg = _config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, "rotate=itq")
    assert rotation_request(cfg) == {"method": "itq", "blocks": 4, "iters": 50}              # one block per concept
    cfg = _config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, "rotate=itq", "rotate_blocks=1", "rotate_iters=7")
    assert rotation_request(cfg) == {"method": "itq", "blocks": 1, "iters": 7}
    for overrides, word in ((["rotate=pca"], "rotate must be itq"), (["rotate_blocks=4"], "without rotate=itq"),
                            (["rotate=itq", "rotate_blocks=5"], "divides nbit = 64"), (["rotate=itq", "rotate_blocks=0"], "rotate_blocks"),
                            (["rotate=itq", "rotate_iters=0"], "rotate_iters"), (["rotate=itq", "rotate_blocks=2.5"], "rotate_blocks")):
        with pytest.raises(ValueError, match=word):
            rotation_request(_config(tmp_path, "search.yaml", main_v2.SEARCH_KEYS, *overrides))
    val = _config(tmp_path, "val.yaml", main_v2.EVAL_KEYS)
    assert val.itq_eval is False and val.itq_blocks is None and val.itq_iters == 50
    val = _config(tmp_path, "val.yaml", main_v2.EVAL_KEYS, "itq_eval=true", "itq_blocks=2")
    assert val.itq_eval is True and check_itq_settings(val.itq_blocks, val.itq_iters, val.model.ncontext) == (2, 50)
    assert check_itq_settings(None, None, 4) == (4, 50)
    for blocks, iters in ((0, 50), (2.5, 50), (True, 50), (4, 0), (4, "x")):
        with pytest.raises(ValueError, match="itq_eval: itq_"):
            check_itq_settings(blocks, iters, 4)


def test_the_evaluator_refuses_what_it_cannot_rotate(monkeypatch):
    import torch.distributed as dist
    import utils.hashing
    from concepthash_amd.distributed import RowShard
    from experiments.itq_eval import rotated_pair
    with pytest.raises(ValueError, match="itq_blocks = 5 does not divide the evaluated code width 32"):
        rotated_pair(torch.zeros(4, 32), torch.zeros(2, 32), 5, 50)
    shard = RowShard.__new__(RowShard)
    with pytest.raises(NotImplementedError, match="one process"):
        utils.hashing._single_process("hamming after itq_eval", shard, None)
    monkeypatch.setattr(utils.hashing, "_sharded", lambda: True)
    with pytest.raises(NotImplementedError, match="one process"):
        utils.hashing._single_process("hamming after itq_eval", torch.zeros(1, 1))


def test_main_v2_runs_the_itq_evaluator_only_when_asked(tmp_path, monkeypatch):
    import main_v2
    import experiments.itq_eval as ie
    import experiments.rerank_eval as re_
    made = []
    for mod, name in ((ie, "ItqEvaluation"), (re_, "RerankEvaluation")):
        cls = type(name, (), {"__init__": lambda self, cfg, n=name: made.append(n), "main": lambda self: None})
        monkeypatch.setattr(mod, name, cls)
    from concepthash_amd import config as cfglib

    def run(*overrides):
        cfg = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml",
                             ["logdir=" + _run_dir(tmp_path), "dataset=synthetic_cub200", "data_dir=" + str(tmp_path)] + list(overrides), cwd=str(tmp_path))
        main_v2.run(cfg)
    run("rerank_eval=true", "itq_eval=true")
    run("rerank_eval=true")
    assert made == ["ItqEvaluation", "RerankEvaluation"]


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_exported_and_bound():
    from concepthash_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "concepthash_hip.h")).read()
    for name in ("ch_itq_step_workspace", "ch_itq_step", "ch_itq_rotate"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert "itq.hip" in build.SOURCES and build.EXTRA_FLAGS["itq.hip"] == ["-ffp-contract=off"]
    # the host-side refusals (status 2, the house messages); rows == 0 is no error and launches nothing
    assert lib.ch_itq_step(None, 5, 300, None, 4, 0, None, None, None, 0, None) == 2 and b"itq_step: n must be in [1, 256]" in lib.ch_last_error()
    assert lib.ch_itq_step(None, 5, 64, None, 5, 0, None, None, None, 0, None) == 2 and b"block must be >= 1 and divide n" in lib.ch_last_error()
    assert lib.ch_itq_step(None, -5, 64, None, 16, 0, None, None, None, 0, None) == 2 and b"negative rows" in lib.ch_last_error()
    assert lib.ch_itq_step(None, 5, 64, None, 16, 0, None, None, None, 0, None) == 2 and b"null pointer" in lib.ch_last_error()
    assert lib.ch_itq_step(None, 5, 64, None, 16, 4097, None, None, None, 0, None) == 2 and b"seg_rows" in lib.ch_last_error()
    assert lib.ch_itq_rotate(None, 5, 0, None, 1, None, None) == 2 and b"itq_rotate: n must be in [1, 256]" in lib.ch_last_error()
    assert lib.ch_itq_rotate(None, 5, 64, None, 16, None, None) == 2 and b"null pointer" in lib.ch_last_error()
    assert lib.ch_itq_step(None, 0, 64, None, 16, 0, None, None, None, 0, None) == 0 and lib.ch_itq_rotate(None, 0, 64, None, 16, None, None) == 0
    # the workspace: per segment two doubles and the n x s fp32 partial; 1M rows -> 977 segments of 1,024 rows
    assert lib.ch_itq_step_workspace(1_000_000, 64, 16, 0) == 977 * (16 + 64 * 16 * 4) + 16
    assert lib.ch_itq_step_workspace(513, 64, 16, 256) == 3 * (16 + 64 * 16 * 4) + 16
