"""CPU: the host side of the search feature -- argument validation of ch_hamming_topk_masked / ch_hamming_subcode_dist (it runs before
anything touches a GPU), retrieval.concept_mask against a bit-by-bit construction, the GalleryIndex file, and the configuration."""
import os

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import build, _lib
    build.build()
    return _lib.load()


def _masked(lib, mask=1, stride=1, Qn=4, G=4, W=1, k=10):
    """the masked entry with dummy non-null pointers where a test needs one (every case below is refused before a pointer is read)"""
    return lib.ch_hamming_topk_masked(None, mask, stride, Qn, None, G, W, k, 0, None, None, None, 0, None)


def test_masked_topk_refuses_bad_arguments_on_the_host(lib):
    assert _masked(lib, mask=None) != 0 and b"q_mask" in lib.ch_last_error()
    for stride in (1, 3, -1):
        assert _masked(lib, stride=stride, W=2) != 0 and b"mask_stride" in lib.ch_last_error()
    assert _masked(lib, stride=5, W=5) != 0 and b"W" in lib.ch_last_error()
    assert _masked(lib, stride=0, W=5) != 0 and b"W" in lib.ch_last_error()
    assert _masked(lib, k=129) != 0 and b"k" in lib.ch_last_error()
    assert _masked(lib, k=0) != 0 and b"k" in lib.ch_last_error()
    # both accepted strides pass the mask checks: with no queries there is nothing to do
    assert _masked(lib, stride=0, Qn=0, W=2) == 0 and _masked(lib, stride=2, Qn=0, W=2) == 0


def test_subcode_dist_refuses_bad_arguments_on_the_host(lib):
    def call(W=1, k=3, nbit=64, nsub=4, Qn=2, G=5):
        return lib.ch_hamming_subcode_dist(None, Qn, None, G, W, None, k, 0, nbit, nsub, None, None)
    assert call(nbit=64, nsub=5) != 0 and b"nsub" in lib.ch_last_error()
    assert call(nbit=64, nsub=0) != 0 and b"nsub" in lib.ch_last_error()
    assert call(W=1, nbit=65, nsub=5) != 0 and b"nbit" in lib.ch_last_error()
    assert call(W=2, nbit=192, nsub=3) != 0 and b"nbit" in lib.ch_last_error()
    assert call(W=5, nbit=64) != 0 and b"W" in lib.ch_last_error()
    assert call(k=0) != 0 and b"k" in lib.ch_last_error()
    assert call(Qn=0) == 0


def _mask_by_bits(nbit, Q, concepts):
    W = (nbit + 63) // 64
    words = [0] * W
    for i in range(nbit):
        if i // (nbit // Q) in concepts:
            words[i // 64] |= 1 << (i % 64)
    return [w - (1 << 64) if w >> 63 else w for w in words]


@pytest.mark.parametrize("nbit,Q", [(64, 4), (48, 4), (120, 3), (256, 4), (16, 4)])
def test_concept_mask_equals_the_bit_by_bit_construction(nbit, Q):
    from concepthash_amd import retrieval as rt
    sets = [[], list(range(Q)), [0], [Q - 1], [1], [0, Q - 1], list(range(Q))[::-1]]
    for cs in sets:
        m = rt.concept_mask(nbit, Q, cs)
        assert m.dtype == torch.int64 and m.shape == ((nbit + 63) // 64,) and not m.is_cuda
        assert m.tolist() == _mask_by_bits(nbit, Q, set(cs)), cs
    full = rt.concept_mask(nbit, Q, range(Q)).tolist()
    assert sum(bin(w & 0xFFFFFFFFFFFFFFFF).count("1") for w in full) == nbit          # bits past nbit stay clear
    assert rt.concept_mask(nbit, Q, []).tolist() == [0] * ((nbit + 63) // 64)
    for bad in ([Q], [-1], [0, 0], [1, 0, 1]):
        with pytest.raises(ValueError):
            rt.concept_mask(nbit, Q, bad)
    with pytest.raises(ValueError):
        rt.concept_mask(nbit, nbit + 1, [0])


def _index(G=7, nbit=120, Q=3, with_paths=True, with_mean=True):
    from concepthash_amd.search import GalleryIndex
    g = torch.Generator().manual_seed(5)
    W = (nbit + 63) // 64
    codes = torch.randint(-2 ** 62, 2 ** 62, (G, W), generator=g, dtype=torch.int64)
    return GalleryIndex(codes, nbit, Q, labels=torch.arange(G) % 3, paths=[f"img/{i}.jpg" for i in range(G)] if with_paths else None,
                        data_root="/data/birds" if with_paths else None, mean=torch.randn(nbit, generator=g) if with_mean else None,
                        transform={"resize": 256, "crop": 224, "norm": 2}, fingerprint={"file": "best.pth", "size": 11, "sha256": "ab" * 32})


@pytest.mark.parametrize("with_paths,with_mean", [(True, True), (False, False)])
def test_gallery_index_round_trip(tmp_path, with_paths, with_mean):
    from concepthash_amd.search import GalleryIndex
    a = _index(with_paths=with_paths, with_mean=with_mean)
    path = str(tmp_path / "sub" / "index.pth")
    a.save(path)
    raw = torch.load(path, map_location="cpu")                 # one plain torch.save file of CPU tensors
    assert raw["format"] == 1 and not raw["codes"].is_cuda and set(raw) == {"format", "codes", "nbit", "ncontext", "labels", "paths",
                                                                            "data_root", "mean", "transform", "fingerprint"}
    b = GalleryIndex.load(path, fingerprint=dict(a.fingerprint), nbit=120)
    assert torch.equal(a.codes, b.codes) and torch.equal(a.labels, b.labels) and (a.nbit, a.ncontext) == (b.nbit, b.ncontext) == (120, 3)
    assert a.paths == b.paths and a.data_root == b.data_root and a.transform == b.transform and a.fingerprint == b.fingerprint
    assert (b.mean is None) == (not with_mean) and (b.mean is None or torch.equal(a.mean, b.mean))
    assert len(b) == 7 and b.device.type == "cpu" and b.to("cpu").paths == a.paths
    assert b.resolve(None) is None
    if with_paths:
        assert b.resolve("img/3.jpg") == "/data/birds/img/3.jpg" and b.resolve("/abs/x.jpg") == "/abs/x.jpg"


def test_gallery_index_refuses_another_checkpoint_or_code_length(tmp_path):
    from concepthash_amd.search import GalleryIndex, StaleIndexError, checkpoint_fingerprint
    a = _index()
    path = str(tmp_path / "index.pth")
    a.save(path)
    with pytest.raises(StaleIndexError, match="rebuild"):
        GalleryIndex.load(path, fingerprint={"file": "best.pth", "size": 11, "sha256": "cd" * 32})
    with pytest.raises(StaleIndexError, match="rebuild"):
        GalleryIndex.load(path, fingerprint={"file": "best.pth", "size": 12, "sha256": "ab" * 32})
    with pytest.raises(StaleIndexError, match="rebuild"):
        GalleryIndex.load(path, fingerprint=dict(a.fingerprint), nbit=64)
    GalleryIndex.load(path, fingerprint={"file": "last.pth", "size": 11, "sha256": "ab" * 32}, nbit=120)   # the same bytes under another name
    torch.save({"codes": a.codes}, path)
    with pytest.raises(StaleIndexError, match="rebuild"):
        GalleryIndex.load(path)
    # the fingerprint is the file's size and sha256
    ck = tmp_path / "best.pth"
    ck.write_bytes(b"abc")
    fp = checkpoint_fingerprint(str(ck))
    assert fp == {"file": "best.pth", "size": 3, "sha256": "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"}
    ck.write_bytes(b"abd")
    assert checkpoint_fingerprint(str(ck))["sha256"] != fp["sha256"]
    # inconsistent pieces are refused when the index is made
    with pytest.raises(ValueError):
        GalleryIndex(a.codes, 64, 4)
    with pytest.raises(ValueError):
        GalleryIndex(a.codes, 120, 7)
    with pytest.raises(ValueError):
        GalleryIndex(a.codes, 120, 3, paths=["x"])


def test_search_and_concept_eval_configuration(tmp_path):
    import main_v2
    from concepthash_amd import config as cfglib
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml",
                         ["logdir=" + str(tmp_path / "run"), "dataset=synthetic_cub200", "concepts=[0,2]", "k=7", "query_margin=0.25"],
                         cwd=str(tmp_path))
    assert cfg.exp == "search" and cfg.k == 7 and cfg.concepts == [0, 2] and cfg.query_margin == 0.25 and cfg.query == "test"
    assert cfg.index is None and cfg.rebuild_index is False and cfg.save_attention is False
    assert cfg.search_logdir.startswith(str(tmp_path / "run" / "searches")) and cfg.dataset.nclass == 200
    assert all(k in cfg for k in main_v2.SEARCH_KEYS)          # main_v2.run lays every one of them over the run's config
    val = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", ["logdir=" + str(tmp_path / "run"), "dataset=synthetic_cub200"],
                         cwd=str(tmp_path))
    assert val.concept_eval is False and "concept_eval" in main_v2.LOOP_KEYS
    # the overlay itself: a run's config.yaml + the command line's keys
    import yaml
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yaml").write_text(yaml.safe_dump({"seed": 7, "model": {"nbit": 64}, "batch_size": 32, "exp": "hashing"}))
    on = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", ["logdir=" + str(run), "dataset=synthetic_cub200", "concept_eval=true"],
                        cwd=str(tmp_path))
    laid = main_v2._run_config(on, "validation", main_v2.EVAL_KEYS)
    assert laid.concept_eval is True and laid.exp == "validation" and laid.model.nbit == 64 and laid.batch_size == 64
    laid = main_v2._run_config(cfg, "search", main_v2.SEARCH_KEYS)
    assert laid.exp == "search" and laid.concepts == [0, 2] and laid.model.nbit == 64 and laid.logdir == str(run)


@pytest.mark.parametrize("tie", [False, True])
def test_concept_evaluation_scores_the_column_slices_the_evaluator_scored(tmp_path, monkeypatch, tie):
    """experiments.concept_eval.ConceptEvaluation around a stub evaluator and a stub metric (no GPU): every calculate_mAP call of the
    evaluator is followed by one per concept on that concept's columns of the SAME codes, the lists land beside the call's own key, the
    tie bracket (when on) stays the whole code's, and the rebound names are restored."""
    import json
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.concept_eval import ConceptEvaluation
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, tie_bracket=False, PRs=None, **k):
        seen.append((tuple(db_codes.shape), tuple(test_codes.shape), bool(tie_bracket)))
        m = float(db_codes.sum() + test_codes.sum())           # a function of exactly the columns handed over
        utils.hashing.last_tie_bracket = {"mAP_low": m - 1, "mAP_high": m + 1} if tie_bracket else None
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
    ev = ConceptEvaluation.__new__(ConceptEvaluation)
    ev.config = _wrap({"concept_eval": True, "compute_mAP": True, "exp": "validation", "tie_bracket": tie, "sub_code_eval": False,
                       "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    want = [float(db[:, a:a + 4].sum() + te[:, a:a + 4].sum()) for a in (0, 4, 8)]
    assert res["mAP_concept"] == want and res["mAP_concept_bin"] == [2 * w for w in want]
    assert res["recalls_concept"] == [[w, w] for w in want] and res["precisions_concept"] == [[-w, -w] for w in want]
    assert res["mAP"] == float(db.sum() + te.sum())
    # per evaluator call: the three slices (never with a bracket), then the whole code
    assert seen == ([((5, 4), (3, 4), False)] * 3 + [((5, 12), (3, 12), tie)]) * 2
    if tie:
        assert res["mAP_tie_low"] == res["mAP"] - 1 and res["mAP_tie_high_bin"] == res["mAP_bin"] + 1
    assert json.load(open(tmp_path / "history.json")) == res
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    ev.config["sub_code_eval"] = True
    with pytest.raises(ValueError, match="sub_code_eval"):
        ev.main()
    ev.config["concept_eval"], ev.config["sub_code_eval"] = False, False     # the key off: the evaluator alone
    assert "mAP_concept" not in ev.main()
