"""GPU: text queries.  ch_model_project_text against the fp64 restatement tests/text_query_ref.py within its
derived bound, its bit-for-bit equality with the load-time fold of the centres, its argument checks; then `exp=search` with text queries
and `exp=validation text_eval=true` on a tiny seeded run: a local HF directory with a two-layer vision half and the two-layer text tower
of tests/test_text_tower_gpu.py (`SMALL`), five ragged class names, and a few hundred synthetic database codes."""
import json
import os

import numpy as np
import pytest
import torch

import text_query_ref as tq
import text_tower_ref as ttr
from conftest import ROOT
from test_text_tower_gpu import SMALL

pytestmark = pytest.mark.gpu

NCLASS = 5                                             # rows of the handle's own `center`: N = 257 goes through 52 chunks of them
VISION = dict(D=128, L=1, heads=2, M=256, patch=16, image=32, P=32, b=128)
CLASS_NAMES = ("001.Black_footed_Albatross", "Brewer's_Blackbird", "warbler", "the_bird_of_the_north", "Quail_10")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _state_dict(cd, nbit, form):
    """a one-layer ViT around text_projection weights of tests/text_query_ref.py; form None: a model without text_projection"""
    from concepthash_amd import synthetic
    sd = synthetic.synthetic_state_dict(VISION, nbit=nbit, nclass=NCLASS, seed=11, center_dim=cd)
    for k in [k for k in sd if k.startswith("text_projection.")]:
        del sd[k]
    if form is not None:
        sd.update(tq.projection_weights(cd, nbit, form))
    return sd


@pytest.fixture(scope="module")
def handles(dev):
    """(cd, nbit, form) -> (encoder, state_dict), built on first use and closed with the module"""
    from concepthash_amd.encoder import ConceptHashEncoder
    made = {}

    def get(cd, nbit, form):
        if (cd, nbit, form) not in made:
            sd = _state_dict(cd, nbit, form)
            made[cd, nbit, form] = (ConceptHashEncoder(sd, heads=VISION["heads"], max_batch=2, device=dev), sd)
        return made[cd, nbit, form]
    yield get
    for enc, _ in made.values():
        enc.close()


def _centers(enc, which):
    cols = enc.cfg["center_dim"] if which == 0 else enc.nbit
    out = torch.empty(enc.cfg["nclass"], cols, dtype=torch.float32, device=enc.device)
    from concepthash_amd import _lib
    _lib.check(enc.lib.ch_debug_model_centers(enc._h, which, _lib.ptr(out), _lib.stream_ptr()), "ch_debug_model_centers")
    return out


# ---- 5. the entry against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tq.FORMS)
@pytest.mark.parametrize("cd", tq.CENTER_DIMS)
@pytest.mark.parametrize("nbit", tq.NBITS)
def test_project_text_is_inside_the_derived_bound(handles, dev, form, cd, nbit):
    from concepthash_amd import retrieval as rt
    enc, sd = handles(cd, nbit, form)
    tp = {k: v for k, v in sd.items() if k.startswith("text_projection.")}
    for N in tq.NS:
        f = tq.features(N, cd)
        z, bound = tq.text_query_ref(f, tp)
        rows = tq.centre_rows(f).to(dev)
        got = enc.project_text(rows)
        torch.cuda.synchronize()
        assert got.shape == (N, nbit) and got.dtype == torch.float32
        g = got.cpu()
        ratio = float(((g.double() - z).abs() / bound).max())
        ok, flips = tq.flips_are_inside_the_bound(g, z, bound)
        print(f"project_text {form} cd={cd} nbit={nbit} N={N}: worst error / bound {ratio:.3f}, sign flips {flips}")
        assert bool(torch.isfinite(g).all()) and not tq.breaches(g, z, bound), (form, cd, nbit, N, ratio)
        assert ok
        # the packed bits are those of the returned code, and a row's result does not depend on the rows around it (N > C: chunks)
        want = np.packbits(np.pad(tq.text_query_bits(g).numpy(), ((0, 0), (0, -nbit % 64))), axis=1, bitorder="little").view(np.uint64)
        assert np.array_equal(rt.pack_sign(got).cpu().numpy().view(np.uint64), want)
        if N > 1:
            assert torch.equal(enc.project_text(rows[N - 1:]).cpu(), g[N - 1:])


# ---- 6. equality with the load-time fold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tq.FORMS)
@pytest.mark.parametrize("cd,nbit", [(64, 12), (512, 64), (64, 128)])
def test_the_models_own_centres_through_the_entry_are_the_folded_centres(handles, dev, form, cd, nbit):
    """The test that fails if ch_model_project_text and the fold of ch_model_create ever drift apart: `center` -> the entry -> the
    normalisation launch of the fold == center_l2 / center_bin of the handle, bit for bit."""
    from concepthash_amd import _lib
    enc, sd = handles(cd, nbit, form)
    center = _centers(enc, 0)
    assert torch.equal(center.cpu(), sd["center"])
    proj = enc.project_text(center)
    l2, bn = torch.empty_like(proj), torch.empty_like(proj)
    _lib.check(enc.lib.ch_debug_small_l2norm(_lib.ptr(proj), NCLASS, nbit, _lib.ptr(l2), _lib.ptr(bn), _lib.stream_ptr()), "l2norm")
    torch.cuda.synchronize()
    assert torch.equal(l2, _centers(enc, 1)) and torch.equal(bn, _centers(enc, 2))
    assert float(l2.abs().max()) > 0 and bool((bn != 0).all())


# ---- 7. argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_a_status_launch_nothing_and_leave_the_handle_usable(handles, dev):
    from concepthash_amd import _lib
    from concepthash_amd.encoder import ConceptHashEncoder
    enc, sd = handles(64, 64, "mlp")
    lib = enc.lib
    rows = tq.centre_rows(tq.features(3, 64)).to(dev)
    out = torch.zeros(3, 64, device=dev)
    sp = _lib.stream_ptr()
    assert lib.ch_model_project_text(enc._h, _lib.ptr(rows), 0, _lib.ptr(out), sp) != 0 and b"N must be >= 1" in lib.ch_last_error()
    assert lib.ch_model_project_text(enc._h, _lib.ptr(rows), -3, _lib.ptr(out), sp) != 0 and b"N must be >= 1" in lib.ch_last_error()
    assert lib.ch_model_project_text(enc._h, None, 3, _lib.ptr(out), sp) != 0 and b"null feats" in lib.ch_last_error()
    assert lib.ch_model_project_text(enc._h, _lib.ptr(rows), 3, None, sp) != 0 and b"out_codes" in lib.ch_last_error()
    assert lib.ch_model_project_text(None, _lib.ptr(rows), 3, _lib.ptr(out), sp) != 0 and b"null model" in lib.ch_last_error()
    # a handle created without text_projection (centres of code width, as LGHWithoutText keeps them): its centres fold as they are
    plain = ConceptHashEncoder(_state_dict(64, 64, None), heads=VISION["heads"], max_batch=2, device=dev)
    try:
        assert lib.ch_model_project_text(plain._h, _lib.ptr(rows), 3, _lib.ptr(out), sp) != 0
        assert b"without text_projection" in lib.ch_last_error()
        with pytest.raises(RuntimeError, match="without text_projection"):
            plain.project_text(rows)
        l2, bn = torch.empty(NCLASS, 64, device=dev), torch.empty(NCLASS, 64, device=dev)
        _lib.check(lib.ch_debug_small_l2norm(_lib.ptr(_centers(plain, 0)), NCLASS, 64, _lib.ptr(l2), _lib.ptr(bn), sp), "l2norm")
        assert torch.equal(l2, _centers(plain, 1)) and torch.equal(bn, _centers(plain, 2))
    finally:
        plain.close()
    with pytest.raises(ValueError, match="text features must be"):
        enc.project_text(rows[:, :63])
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                # nothing was launched
    z, bound = tq.text_query_ref(tq.features(3, 64), {k: v for k, v in sd.items() if k.startswith("text_projection.")})
    assert not tq.breaches(enc.project_text(rows).cpu(), z, bound)


# ---- 8 and 9: a tiny run ---------------------------------------------------------------------------------------------------------------
def _compose(name, tmp, *overrides):
    from concepthash_amd import config as cfglib
    return cfglib.compose(os.path.join(ROOT, "configs"), name,
                          ["dataset=synthetic_cub200", "dataset.nclass=5", "dataset.crop=32", "dataset.limit=48", "data_dir=" + str(tmp),
                           "batch_size=16"] + list(overrides), cwd=str(tmp))


@pytest.fixture(scope="module")
def run(tmp_path_factory, dev):
    """A local HF CLIP directory (vision 128 x 2 at 32 x 32 pixels, the SMALL text tower, tokeniser files), class_names.txt, a run
    directory whose seeded checkpoint keeps the language-guided centres the model was built with, and a gallery index of 300
    synthetic codes with labels."""
    from safetensors.torch import save_file
    from concepthash_amd import config as cfglib, retrieval as rt
    from concepthash_amd.search import GalleryIndex, checkpoint_fingerprint
    from models.backbone.clip import CLIPModelShell
    tmp = tmp_path_factory.mktemp("text_query")
    clip = tmp / "clip"
    clip.mkdir()
    vocab, _ = ttr.write_tokenizer_files(str(clip))
    dims = dict(SMALL, vocab_size=len(vocab))
    vis = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, patch_size=16, image_size=32)
    eos = vocab["<|endoftext|>"]
    with open(clip / "config.json", "w") as f:
        json.dump({"model_type": "clip", "projection_dim": 32, "vision_config": dict(vis, hidden_act="quick_gelu"),
                   "text_config": dict(dims, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=eos, pad_token_id=eos,
                                       bos_token_id=vocab["<|startoftext|>"])}, f)
    torch.manual_seed(5)
    shell = CLIPModelShell(dict(vis, projection_dim=32, hidden_act="quick_gelu")).state_dict()
    weights = {k: v.contiguous() for k, v in shell.items() if not k.startswith("text_projection") and k != "logit_scale"}
    weights.update({k: v.contiguous() for k, v in ttr.seeded_text_state_dict(dims, seed=9).items()})
    save_file(weights, str(clip / "model.safetensors"))
    folder = tmp / "data" / "cub200_2011"
    folder.mkdir(parents=True)
    (folder / "class_names.txt").write_text("\n".join(CLASS_NAMES) + "\n")
    # the run: train.yaml composed for this backbone, centres 128 wide (the text tower's width), built by instantiating the model
    logdir = tmp / "run"
    cfg = _compose("train.yaml", tmp, "logdir=" + str(logdir), "model.backbone.name=" + str(clip), "model.nbit=64", "model.fixed_center.dim=128")
    cfg.model.text_projection._args_[0].in_features = cfg.model.text_projection._args_[0].out_features = 128
    cfg.model.text_projection._args_[2].in_features = 128
    (logdir / "models").mkdir(parents=True)
    with open(logdir / "config.yaml", "w") as f:
        import yaml
        yaml.safe_dump(cfglib.to_container(cfg), f)
    torch.manual_seed(int(cfg.seed))
    model = cfglib.instantiate(cfg.model)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("up_proj.weight"):
                p.normal_(0, 0.02)
        for lin in (model.text_projection[0], model.text_projection[2]):
            lin.weight.normal_(0, 128 ** -0.5)
            lin.bias.normal_(0, 0.5)
        model.hash_bn.running_mean.normal_(0, 0.1)
        model.hash_bn.running_var.uniform_(0.5, 1.5)
    assert tuple(model.center.shape) == (5, 128) and bool((model.center.abs() == 1).all())     # language-guided, not the seeded fallback
    torch.save(model.state_dict(), str(logdir / "models" / "best.pth"))
    g = torch.Generator().manual_seed(3)
    labels = torch.arange(300) % 5
    db = torch.randn(300, 64, generator=g)
    ds = cfg.dataset
    index = GalleryIndex(rt.pack_sign(db.to(dev)), 64, 4, labels=labels, transform={"resize": int(ds.resize), "crop": int(ds.crop), "norm": int(ds.norm)},
                         fingerprint=checkpoint_fingerprint(str(logdir / "models" / "best.pth")))
    index.save(str(logdir / "index_best.pth"))
    return dict(tmp=tmp, logdir=str(logdir), clip=str(clip), names=str(folder / "class_names.txt"), labels=labels)


def _search(run, name, **keys):
    """exp=search as main_v2.run starts it -> (the experiment, results.json)"""
    import main_v2
    from experiments.search import SearchExperiment
    out = str(run["tmp"] / name)
    cfg = _compose("search.yaml", run["tmp"], "logdir=" + run["logdir"], "search_logdir=" + out)
    for k, v in keys.items():
        cfg[k] = v
    assert cfg.exp == "search"
    ex = SearchExperiment(main_v2._run_config(cfg, "search", main_v2.SEARCH_KEYS))
    ex.main()
    return ex, json.load(open(os.path.join(out, "results.json")))


def test_search_by_class_prompts_equals_search_by_the_folded_centres(run, dev):
    """`exp=search query=classes` hit for hit against `index.search` on the model's own `center` rows through ch_model_project_text, for
    the whole code, two concepts, the asymmetric ranking and a deep list inside a radius; then `query_text` of the same strings.  The
    checkpoint is seeded, not trained: what is tested is that text queries ARE centre queries -- retrieval quality itself cannot be
    tested without a trained model."""
    from trainers.orthohash import class_prompts
    prompts = class_prompts(run["names"], "a photo of a ")
    variants = [dict(k=7), dict(k=7, concepts=[0, 2]), dict(k=7, rank="asymmetric"), dict(k=200, radius=40)]
    first = None
    for i, v in enumerate(variants):
        ex, res = _search(run, f"s{i}", query="classes", **v)
        first = first or res
        model, index = ex.trainer.model, ex.index.to(dev)
        assert ex.trainer.dataset is None                                   # a valid index: no dataset of the run was loaded
        assert res["index_status"] == "loaded" and "encode_db" not in res["timing_s"] and "datasets" not in res["timing_s"]
        assert res["query_kind"] == "text" and res["query"] == prompts and res["prefix"] == "a photo of a " and res["text_model"] == run["clip"]
        assert res["center_agreement"] == 1.0 and res["mean_shift"] is False and res["index_rows"] == 300
        codes = model.project_text(model.center)
        want = index.search(codes, v["k"], v.get("concepts"), 0.0, v.get("rank", "hamming"), 8, v.get("radius"), mean_shift=False)
        idx, dist = want["idx"].tolist(), want["dist"].tolist()
        assert len(res["queries"]) == 5
        for c, e in enumerate(res["queries"]):
            n = sum(1 for x in idx[c] if x >= 0)
            assert e["query"] == prompts[c] and e["label"] == c
            assert [h["index"] for h in e["hits"]] == idx[c][:n] and [h["distance"] for h in e["hits"]] == dist[c][:n], (v, c)
            assert all(h["label"] == int(run["labels"][h["index"]]) and h["relevant"] == (h["label"] == c) for h in e["hits"])
            if "radius" in v:
                assert 7 < n <= 200 and all(h["distance"] <= 40 for h in e["hits"])
            else:
                assert n == 7
    # the same strings as free text: the same hits, no label
    ex, res = _search(run, "free", query_text=prompts, prompt_prefix="", k=7)
    assert res["query_kind"] == "text" and res["query"] == prompts and res["prefix"] == "" and res["center_agreement"] == 1.0
    for e, w in zip(res["queries"], first["queries"]):
        assert e["label"] is None and e["query"] == w["query"]
        assert [(h["index"], h["distance"], h["concept_distances"]) for h in e["hits"]] == [(h["index"], h["distance"], h["concept_distances"])
                                                                                             for h in w["hits"]]
        assert all(h["relevant"] is None for h in e["hits"])


def test_class_prompts_give_the_bits_logits_bin_is_computed_against(run, dev):
    """Consequence 1 of the definition: the prompt of class c yields exactly the bits of sign(get_center()[c]) -- up to entries of
    get_center() that torch and the library round to different sides of zero, i.e. smaller than the derived bound."""
    from concepthash_amd import config as cfglib
    from concepthash_amd.text import TextQueryEncoder
    cfg = cfglib.load(os.path.join(run["logdir"], "config.yaml"))
    model = cfglib.instantiate(cfg.model)
    model.load_state_dict(torch.load(os.path.join(run["logdir"], "models", "best.pth"), map_location="cpu"))
    model = model.to(dev)
    from trainers.orthohash import class_prompts
    with TextQueryEncoder(model, run["clip"]) as enc, torch.no_grad():
        codes = enc.text_codes(class_prompts(run["names"], ""))             # the bare names under the object's default prefix
        assert enc.center_agreement(run["names"]) == 1.0
        assert enc.center_agreement(run["names"], prefix="a drawing of the ") < 1.0      # another prefix: reported, not refused
        assert enc.tower is not None
    assert enc.tower is None                                                 # closed with the block
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith("text_projection.")}
    z, bound = tq.text_query_ref(model.center.cpu(), sd)                     # the centres are +-1: centre_rows leaves them as they are
    assert not tq.breaches(codes.cpu(), z, bound)
    ref_bits = model.get_center().detach().cpu() > 0
    diff = (codes.cpu() > 0) != ref_bits
    assert bool((z.abs()[diff] <= bound[diff]).all())


def test_text_eval_adds_the_text_scores_and_leaves_the_rest(run, dev):
    """`exp=validation text_eval=true`: mAP_text / recalls_text / precisions_text equal a direct calculate_mAP of the class prompts' codes
    (eye(C) labels) against the database codes the run saved, and every other key equals that of a run without the flag."""
    import main_v2
    from utils.hashing import calculate_mAP
    outs = {}
    for name, extra in (("with", ["text_eval=true", "save_code=True"]), ("without", [])):
        ev = str(run["tmp"] / ("ev_" + name))
        cfg = _compose("val.yaml", run["tmp"], "logdir=" + run["logdir"], "eval_logdir=" + ev, *extra)
        main_v2.run(cfg)
        outs[name] = json.load(open(os.path.join(ev, "history.json")))
    on, off = outs["with"], outs["without"]
    assert not [k for k in off if "text" in k or k == "center_agreement"]
    new = {"mAP_text", "recalls_text", "precisions_text", "center_agreement", "text_prompt_prefix", "text_model"}
    assert set(on) - set(off) == new and on["center_agreement"] == 1.0
    assert {k: v for k, v in on.items() if k not in new and k != "timing_s"} == {k: v for k, v in off.items() if k != "timing_s"}
    assert {"encode_text", "retrieval_text"} <= set(on["timing_s"])
    saved = torch.load(os.path.join(str(run["tmp"] / "ev_with"), "outputs.pth"))
    db_codes, db_labels = saved["db"]["codes"], saved["db"]["labels"]
    if db_labels.dim() == 1:
        db_labels = torch.nn.functional.one_hot(db_labels, 5)
    from concepthash_amd import config as cfglib
    model = cfglib.instantiate(cfglib.load(os.path.join(run["logdir"], "config.yaml")).model)
    model.load_state_dict(torch.load(os.path.join(run["logdir"], "models", "best.pth"), map_location="cpu"))
    model = model.to(dev)
    text_codes = model.project_text(model.center).cpu()
    m, r, p = calculate_mAP(db_codes, db_labels, text_codes, torch.eye(5, dtype=db_labels.dtype), -1, PRs=[1, 5, 10])
    assert (on["mAP_text"], on["recalls_text"], on["precisions_text"]) == (m, r, p)
    assert len(r) == len(p) == 3 and 0.0 <= m <= 1.0
