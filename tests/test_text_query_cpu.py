"""CPU: the host side of text queries -- the fp64 restatement of steps 3-5 and its derived bound against an fp32
emulation with and without named defects, the configuration keys, the argument errors (all raised before anything touches a GPU: there
is none here, so a RuntimeError about a missing GPU in their place fails the test) and the prompt building."""
import os

import pytest
import torch
import yaml

import text_query_ref as tq
from conftest import ROOT

FIXED = "models.arch.coop.LGHWithFixedPrompt"


# ---- 1. the restatement and its bound -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tq.FORMS)
@pytest.mark.parametrize("cd", tq.CENTER_DIMS)
@pytest.mark.parametrize("nbit", tq.NBITS)
def test_the_bound_holds_a_clean_emulation_and_every_defect_leaves_it(form, cd, nbit):
    sd = tq.projection_weights(cd, nbit, form)
    for N in tq.NS:
        f = tq.features(N, cd)
        z, bound = tq.text_query_ref(f, sd)
        assert z.shape == bound.shape == (N, nbit) and z.dtype == torch.float64 and bool((bound > 0).all())
        # the bound is a rounding bound, not a tolerance: far below the values it guards (their RMS is ~1)
        assert float(bound.max()) < 1e-3 * float(z.pow(2).mean().sqrt())
        clean = tq.text_query_emul(f, sd)
        assert clean.dtype == torch.float32 and not tq.breaches(clean, z, bound), (form, cd, nbit, N)
        ok, _ = tq.flips_are_inside_the_bound(clean, z, bound)
        assert ok
        for defect in tq.DEFECTS[form]:
            if defect == "wrong_prompt" and N == 1:
                continue                                   # one prompt has no neighbour to be mistaken for
            assert tq.breaches(tq.text_query_emul(f, sd, defect), z, bound), (form, cd, nbit, N, defect)


def test_zero_features_stay_zero_centre_entries_and_bits_are_strict():
    f = tq.features(3, 64)
    c = tq.centre_rows(f)
    assert bool((f == 0).any()) and torch.equal(c == 0, f == 0) and set(c.unique().tolist()) == {-1.0, 0.0, 1.0}
    # get_codebook("L") makes its rows through the same function
    import trainers.orthohash as oh
    assert torch.equal(oh.centre_rows(f), f.sign())
    z = torch.tensor([[0.0, -0.0, 1e-30, -1e-30]], dtype=torch.float64)
    assert tq.text_query_bits(z).tolist() == [[False, False, True, False]]


# ---- fixtures of the configuration tests ------------------------------------------------------------------------------------------------
def _text_dir(path):
    """what `local_text_files` looks for (existence only: nothing here reads the files)"""
    os.makedirs(path)
    for name in ("config.json", "model.safetensors", "vocab.json", "merges.txt"):
        open(os.path.join(path, name), "w").close()
    return str(path)


def _run_dir(tmp_path, backbone, target=FIXED, prefix="a photo of a "):
    run = tmp_path / "run"
    run.mkdir(exist_ok=True)
    (run / "config.yaml").write_text(yaml.safe_dump({
        "seed": 7, "batch_size": 32, "exp": "hashing", "trainer": {"_target_": "trainers.coop.COOPTrainer"},
        "model": {"_target_": target, "nbit": 64, "ncontext": 4, "backbone": {"name": backbone},
                  "fixed_center": {"prompt_prefix": prefix}}}))
    return str(run)


def _search_config(tmp_path, logdir, *overrides):
    import main_v2
    from concepthash_amd import config as cfglib
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml",
                         ["logdir=" + logdir, "dataset=synthetic_cub200", "data_dir=" + str(tmp_path), "search_logdir=" + str(tmp_path / "s")]
                         + list(overrides), cwd=str(tmp_path))
    return main_v2._run_config(cfg, "search", main_v2.SEARCH_KEYS)


def _val_config(tmp_path, logdir, *overrides):
    import main_v2
    from concepthash_amd import config as cfglib
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml",
                         ["logdir=" + logdir, "dataset=synthetic_cub200", "data_dir=" + str(tmp_path), "eval_logdir=" + str(tmp_path / "e")]
                         + list(overrides), cwd=str(tmp_path))
    return main_v2._run_config(cfg, "validation", main_v2.EVAL_KEYS)


def _class_names(tmp_path, lines=("001.Black_footed_Albatross", "Brewer's_Blackbird", "warbler", "the_bird_of_the_north", "Quail_10")):
    folder = tmp_path / "data" / "cub200_2011"
    folder.mkdir(parents=True, exist_ok=True)
    (folder / "class_names.txt").write_text("\n".join(lines) + "\n")
    return str(folder / "class_names.txt")


# ---- 2. configuration -------------------------------------------------------------------------------------------------------------------
def test_the_new_keys_compose_and_default_to_the_image_path(tmp_path):
    import main_v2
    from concepthash_amd import config as cfglib
    from experiments.search import text_request
    base = ["logdir=" + str(tmp_path / "run"), "dataset=synthetic_cub200"]
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", base, cwd=str(tmp_path))
    for key in ("query_text", "query_text_file", "prompt_prefix", "text_model"):
        assert key in cfg and cfg[key] is None and key in main_v2.SEARCH_KEYS
    assert cfg.query == "test" and all(k in cfg for k in main_v2.SEARCH_KEYS)
    assert text_request(cfg) is None                                    # the defaults: image queries, nothing about text is looked at
    on = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml",
                        base + ['query_text=["a painted bunting","a red car"]', 'prompt_prefix="a picture of a "', "text_model=/models/clip", "k=7"],
                        cwd=str(tmp_path))
    assert list(on.query_text) == ["a painted bunting", "a red car"] and on.prompt_prefix == "a picture of a " and on.text_model == "/models/clip"
    one = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", base + ["query_text=a painted bunting", "query=test"], cwd=str(tmp_path))
    assert one.query_text == "a painted bunting"
    val = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", base, cwd=str(tmp_path))
    assert val.text_eval is False and val.prompt_prefix is None and val.text_model is None
    assert {"text_eval", "prompt_prefix", "text_model"} <= set(main_v2.LOOP_KEYS)
    von = cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", base + ["text_eval=true"], cwd=str(tmp_path))
    assert von.text_eval is True
    # the overlay onto a run's config
    logdir = _run_dir(tmp_path, "openai/clip-vit-base-patch16")
    laid = _val_config(tmp_path, logdir, "text_eval=true", "text_model=/models/clip")
    assert laid.text_eval is True and laid.text_model == "/models/clip" and laid.model.nbit == 64
    laid = _search_config(tmp_path, logdir)
    assert laid.query_text is None and text_request(laid) is None


def test_main_v2_runs_the_text_evaluator_only_when_asked(tmp_path, monkeypatch):
    import main_v2
    import experiments.test_hashing as base
    import experiments.text_eval as te
    made = []
    monkeypatch.setattr(base.RetrievalEvaluation, "__init__", lambda self, config: made.append(type(self).__name__))
    monkeypatch.setattr(te.TextEvaluation, "main", lambda self: "text")
    monkeypatch.setattr(base.RetrievalEvaluation, "main", lambda self: "plain")
    from concepthash_amd import config as cfglib
    d = _text_dir(tmp_path / "clip")
    logdir = _run_dir(tmp_path, d)
    _class_names(tmp_path)
    args = ["logdir=" + logdir, "dataset=synthetic_cub200", "data_dir=" + str(tmp_path), "eval_logdir=" + str(tmp_path / "e")]
    assert main_v2.run(cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", args, cwd=str(tmp_path))) == "plain"
    assert main_v2.run(cfglib.compose(os.path.join(ROOT, "configs"), "val.yaml", args + ["text_eval=true"], cwd=str(tmp_path))) == "text"
    assert made == ["RetrievalEvaluation", "TextEvaluation"]


# ---- 3. argument errors, all before a GPU is touched --------------------------------------------------------------------------------
def test_search_refuses_bad_text_requests_before_anything_is_loaded(tmp_path):
    from experiments.search import SearchExperiment
    d = _text_dir(tmp_path / "clip")
    logdir = _run_dir(tmp_path, d)
    _class_names(tmp_path)
    with pytest.raises(ValueError, match="query_text.*query='db'"):
        SearchExperiment(_search_config(tmp_path, logdir, "query_text=a bird", "query=db"))
    with pytest.raises(ValueError, match="query=.classes"):
        SearchExperiment(_search_config(tmp_path, logdir, "query_text=a bird", "query=classes"))
    with pytest.raises(ValueError, match="ONE of"):
        SearchExperiment(_search_config(tmp_path, logdir, "query_text=a bird", "query_text_file=" + str(tmp_path / "q.txt")))
    for text in (["query_text=a bird"], ["query=classes"]):
        with pytest.raises(ValueError, match="save_attention.*no image"):
            SearchExperiment(_search_config(tmp_path, logdir, "save_attention=true", *text))
    with pytest.raises(ValueError, match="q.txt does not exist"):
        SearchExperiment(_search_config(tmp_path, logdir, "query_text_file=" + str(tmp_path / "q.txt")))
    (tmp_path / "q.txt").write_text("\n  \n")
    with pytest.raises(ValueError, match="no prompt"):
        SearchExperiment(_search_config(tmp_path, logdir, "query_text_file=" + str(tmp_path / "q.txt")))
    os.remove(tmp_path / "data" / "cub200_2011" / "class_names.txt")
    with pytest.raises(ValueError, match="class_names.txt, which does not exist"):
        SearchExperiment(_search_config(tmp_path, logdir, "query=classes"))


def test_one_error_names_everything_a_run_lacks_for_text(tmp_path):
    from concepthash_amd.text import TextQueryEncoder, text_query_settings
    from experiments.search import SearchExperiment
    from experiments.text_eval import TextEvaluation
    d = _text_dir(tmp_path / "clip")
    hub = _run_dir(tmp_path, "openai/clip-vit-base-patch16")                        # a hub name: no local text tower
    for make in (lambda: SearchExperiment(_search_config(tmp_path, hub, "query_text=a bird")),
                 lambda: SearchExperiment(_search_config(tmp_path, hub, "query=classes")),
                 lambda: TextEvaluation(_val_config(tmp_path, hub, "text_eval=true"))):
        with pytest.raises(ValueError, match="openai/clip-vit-base-patch16.*model.backbone.name.*not a local HF CLIP directory"):
            make()
    # the override is what is checked, and named, when given; a directory that lacks the tokeniser files is not enough
    os.remove(os.path.join(d, "merges.txt"))
    with pytest.raises(ValueError, match="clip' \\(text_model\\) is not a local HF CLIP directory"):
        SearchExperiment(_search_config(tmp_path, hub, "query_text=a bird", "text_model=" + d))
    open(os.path.join(d, "merges.txt"), "w").close()
    assert text_query_settings(_search_config(tmp_path, hub, "text_model=" + d), d) == (d, "a photo of a ")
    # a model without text_projection
    plain = _run_dir(tmp_path, d, target="models.arch.coop.LGHWithoutText")
    with pytest.raises(ValueError, match="LGHWithoutText.*no text_projection"):
        SearchExperiment(_search_config(tmp_path, plain, "query_text=a bird"))
    # both at once: ONE error that names both
    both = _run_dir(tmp_path, "openai/clip-vit-base-patch16", target="models.arch.coop.LGHWithoutText")
    with pytest.raises(ValueError, match="not a local HF CLIP directory.*no text_projection"):
        SearchExperiment(_search_config(tmp_path, both, "query_text=a bird"))
    with pytest.raises(ValueError, match="not a local HF CLIP directory.*no text_projection"):
        TextEvaluation(_val_config(tmp_path, both, "text_eval=true"))
    # the object itself checks what it is given, before it opens a tower
    with pytest.raises(ValueError, match="not a local HF CLIP directory.*Linear.*no text_projection"):
        TextQueryEncoder(torch.nn.Linear(2, 2), str(tmp_path / "missing"))


def test_text_eval_refuses_what_it_cannot_score_before_anything_is_loaded(tmp_path):
    from experiments.text_eval import TextEvaluation
    d = _text_dir(tmp_path / "clip")
    logdir = _run_dir(tmp_path, d)
    with pytest.raises(ValueError, match="class_names.txt, which does not exist"):
        TextEvaluation(_val_config(tmp_path, logdir, "text_eval=true"))
    _class_names(tmp_path)
    for key in ("sub_code_eval", "test_as_database"):
        with pytest.raises(ValueError, match=key):
            TextEvaluation(_val_config(tmp_path, logdir, "text_eval=true", key + "=True"))
    with pytest.raises(ValueError, match="compute_mAP"):
        TextEvaluation(_val_config(tmp_path, logdir, "text_eval=true", "compute_mAP=False"))


def test_multi_rank_groups_are_refused_before_any_encoding(tmp_path, monkeypatch):
    import torch.distributed as dist
    from experiments.search import SearchExperiment
    from experiments.text_eval import TextEvaluation
    d = _text_dir(tmp_path / "clip")
    logdir = _run_dir(tmp_path, d)
    _class_names(tmp_path)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    for text in (["query_text=a bird"], ["query=classes"], ["query_text_file=" + str(tmp_path / "q.txt")]):
        with pytest.raises(NotImplementedError, match="multi-rank"):
            SearchExperiment(_search_config(tmp_path, logdir, *text))
    with pytest.raises(NotImplementedError, match="text_eval under a multi-rank"):
        TextEvaluation(_val_config(tmp_path, logdir, "text_eval=true"))


# ---- 4. prompt building -----------------------------------------------------------------------------------------------------------------
def test_prompts_of_every_text_query_kind(tmp_path):
    from experiments.search import text_request
    from trainers.orthohash import class_prompts
    d = _text_dir(tmp_path / "clip")
    logdir = _run_dir(tmp_path, d, prefix="a photo of a")
    names = _class_names(tmp_path)
    req = text_request(_search_config(tmp_path, logdir, "query=classes"))
    assert req["prompts"] == class_prompts(names, "a photo of a") and req["labels"] == [0, 1, 2, 3, 4]
    assert req["prompts"][0] == "a photo of a 001.Black footed Albatross" and req["prefix"] == req["run_prefix"] == "a photo of a" and req["text_model"] == d
    bare = text_request(_search_config(tmp_path, logdir, "query=classes", 'prompt_prefix=""'))
    assert bare["prefix"] == "" and bare["run_prefix"] == "a photo of a" and bare["prompts"] == class_prompts(names, "")
    assert bare["prompts"] == ["001.Black footed Albatross", "Brewer's Blackbird", "warbler", "the bird of the north", "Quail 10"]
    other = text_request(_search_config(tmp_path, logdir, "query=classes", "prompt_prefix=a sketch of the"))
    assert other["prompts"] == class_prompts(names, "a sketch of the") and other["prompts"][2] == "a sketch of the warbler"
    # query_text / query_text_file: the definition's `prefix + s`, no label
    one = text_request(_search_config(tmp_path, logdir, "query_text=painted bunting", 'prompt_prefix="a photo of a "'))
    assert one["prompts"] == ["a photo of a painted bunting"] and one["labels"] is None
    many = text_request(_search_config(tmp_path, logdir, 'query_text=["a photo of a painted bunting","red car"]', 'prompt_prefix=""'))
    assert many["prompts"] == ["a photo of a painted bunting", "red car"] and many["prefix"] == ""
    (tmp_path / "q.txt").write_text("painted bunting\n\n  red car  \n")
    filed = text_request(_search_config(tmp_path, logdir, "query_text_file=" + str(tmp_path / "q.txt")))
    assert filed["prompts"] == ["a photo of apainted bunting", "a photo of ared car"]      # literally prefix + s: the run's prefix has no space
    from concepthash_amd.text import TextQueryEncoder
    enc = TextQueryEncoder.__new__(TextQueryEncoder)
    enc.prefix = "a photo of a "
    assert enc.prompts("x") == ["a photo of a x"] and enc.prompts(["x", "y"], prefix="") == ["x", "y"]
    with pytest.raises(ValueError, match="no prompt"):
        enc.prompts([])


def test_text_evaluation_scores_the_class_prompts_beside_the_evaluators_own_call(tmp_path, monkeypatch):
    """experiments.text_eval.TextEvaluation around a stub evaluator, a stub metric and a stub encoder (no GPU): the class prompts are
    scored against the database codes of the evaluator's whole-code Hamming call with its R and PRs, labels = eye(C); the bookkeeping
    arguments of the evaluators in between do not reach that call, their left-behind results survive it, and the names are restored."""
    import json
    import experiments.test_hashing as base
    import experiments.text_eval as te
    import concepthash_amd.text as ct
    import utils.hashing
    from concepthash_amd.config import _wrap
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, PRs=None, **k):
        seen.append((tuple(db_codes.shape), tuple(test_codes.shape), R, sorted(k)))
        utils.hashing.last_tie_bracket = {"who": len(seen)}
        m = float(db_codes.sum() + test_codes.sum() + test_labels.sum())
        return m, [m] * len(PRs), [-m] * len(PRs)
    monkeypatch.setattr(utils.hashing, "calculate_mAP", metric)
    monkeypatch.setattr(base, "calculate_mAP", metric)
    db, te_codes = torch.arange(6 * 8, dtype=torch.float32).reshape(6, 8), torch.ones(3, 8)
    db_labels = torch.eye(5)[[0, 1, 2, 3, 4, 0]]

    def evaluator_main(self):
        res = {"timing_s": {}}
        base.calculate_mAP(db[:, :2], db_labels, te_codes[:, :2], db_labels[:3], -1, PRs=[1, 5], threshold=0)       # a concept slice
        res["mAP"], res["recalls"], res["precisions"] = base.calculate_mAP(db, db_labels, te_codes, db_labels[:3], -1, PRs=[1, 5], threshold=0,
                                                                           tie_bracket=True, remove_first_retrieved=False)
        base.calculate_mAP(db, db_labels, te_codes, db_labels[:3], -1, PRs=[1, 5], threshold=0, rank="asymmetric", weight_bits=8)
        self.results = res
        return res
    monkeypatch.setattr(base.RetrievalEvaluation, "main", evaluator_main)
    names = _class_names(tmp_path)
    text_codes = torch.full((5, 8), 0.5)

    class Encoder:
        def __init__(self, model, source, prefix):
            assert (source, prefix) == ("/clip", "")
        __enter__ = lambda self: self
        __exit__ = lambda self, *a: None
        text_codes = lambda self, prompts: (text_codes if prompts[2] == "a photo of a warbler" and len(prompts) == 5 else None)
        center_agreement = lambda self, path, prefix: 0.75 if (path, prefix) == (names, "a photo of a ") else None
    monkeypatch.setattr(ct, "TextQueryEncoder", Encoder)
    ev = te.TextEvaluation.__new__(te.TextEvaluation)
    ev.config = _wrap({"text_eval": True, "compute_mAP": True, "exp": "validation", "model": {"nbit": 8, "ncontext": 4}, "dataset": {"nclass": 5}})
    ev.text = ("/clip", "a photo of a ", names, "a photo of a ")
    ev.rank, ev.eval_logdir, ev.timing = 0, str(tmp_path), {}
    ev._phase = lambda name, fn, *a, **k: (ev.timing.__setitem__(name, 0.0), fn(*a, **k))[1]
    ev.trainer = type("T", (), {"model": torch.nn.Identity()})()
    res = ev.main()
    want = float(db.sum() + text_codes.sum() + 5)
    assert res["mAP_text"] == want and res["recalls_text"] == [want, want] and res["precisions_text"] == [-want, -want]
    assert res["center_agreement"] == 0.75 and res["mAP"] == float(db.sum() + te_codes.sum() + 3)
    assert seen[-1] == ((6, 8), (5, 8), -1, ["threshold"]) and len(seen) == 4
    assert utils.hashing.last_tie_bracket == {"who": 3}                      # what the last call of the evaluators left, not the text call's
    assert json.load(open(tmp_path / "history.json")) == res and set(res["timing_s"]) == {"encode_text", "retrieval_text"}
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    ev.text = None
    assert "mAP_text" not in ev.main()
