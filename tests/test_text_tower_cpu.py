"""CPU: the text tower's torch restatement against transformers, the tokeniser against transformers, the codebook entry point, and the
host-side config checks of ch_text_create.  (The HIP chain itself: tests/test_text_tower_gpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

import text_tower_ref as ttr

DIMS = dict(vocab_size=64, max_position_embeddings=77, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)


def _prompt_ids(B, T, vocab, eos, pad, seed):
    """BOS, words, EOS at a different place in every row, then `pad`; word ids avoid the EOS id"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 1, (B, T), generator=g)
    ids[ids == eos] = 4
    ids[:, 0] = 1 if eos != 1 else 0
    for b in range(B):
        e = max(1, T - 1 - 2 * b)
        ids[b, e] = eos
        ids[b, e + 1:] = pad
    return ids


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("eos_token_id, pad", [(2, 0), (63, 63), (7, 7)])
def test_restatement_matches_transformers(act, eos_token_id, pad):
    """tests/text_tower_ref.py vs transformers' CLIPTextModel (eager attention), seeded weights: last_hidden_state and pooler_output
    within 2e-5 (the suite's oracle-vs-golden tolerance).  eos_token_id 2 = the legacy argmax rule (EOS is then the LARGEST id, 63,
    in the ids); 63 and 7 = the first-match rule with the padding id equal to the EOS id, 7 being smaller than the word ids so
    that argmax(ids) would pick another row."""
    tf = pytest.importorskip("transformers")
    sd = ttr.seeded_text_state_dict(DIMS, seed=3)
    cfg = tf.CLIPTextConfig(**DIMS, hidden_act=act, eos_token_id=eos_token_id, pad_token_id=pad, bos_token_id=1, attn_implementation="eager")
    model = tf.CLIPTextModel(cfg).eval()
    own = set(model.state_dict())         # CLIPTextModel's own keys carry the `text_model.` prefix only in older transformers
    strip = 0 if ttr.TM + "final_layer_norm.weight" in own else len(ttr.TM)
    missing, unexpected = model.load_state_dict({k[strip:]: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing)
    eos_in_ids = 63 if eos_token_id == 2 else eos_token_id
    ids = _prompt_ids(4, 19, 63 if eos_token_id == 2 else 64, eos_in_ids, pad, seed=5)
    with torch.no_grad():
        out = model(input_ids=ids)
    hidden, pooled = ttr.text_forward(sd, ids, heads=2, act=act, eos_token_id=eos_token_id)
    assert (hidden - out.last_hidden_state).abs().max() < 2e-5
    assert (pooled - out.pooler_output).abs().max() < 2e-5
    if pad == eos_in_ids:      # the pooled row is the FIRST EOS, not the last padding position
        first = (ids == eos_in_ids).int().argmax(-1)
        assert (first < ids.shape[1] - 1).any()
        assert torch.equal(pooled, hidden[torch.arange(4), first])


def test_eos_positions_rules():
    from concepthash_amd.text import eos_positions
    ids = np.array([[60, 5, 9, 61, 61, 61], [60, 61, 3, 3, 3, 3], [60, 8, 8, 8, 8, 61]])
    assert eos_positions(ids, 61).tolist() == [3, 1, 5]
    assert eos_positions(ids, 2).tolist() == [3, 1, 5]             # legacy rule: argmax, first of equal maxima
    assert eos_positions(np.array([[9, 4, 2, 7, 2]]), 2).tolist() == [0]
    assert eos_positions(np.array([[9, 4, 3, 7, 3]]), 3).tolist() == [2]
    for e in (2, 61):
        assert eos_positions(ids, e).tolist() == ttr.eos_positions(torch.from_numpy(ids), e).tolist()


PROMPTS = ["a photo of a Black_footed_Albatross".replace("_", " "), "a photo of a  Brewer's   Blackbird", "a photo of a 100 year old BIRD",
           "a photo of a bird", "a photo of a warbler and the blue-winged teal, no. 10!", "a photo of a quail's queue",
           "a photo of a " + "the long bird of the north and the sea " * 12, "  bird  ", "x"]


def test_tokenizer_matches_transformers(tmp_path):
    """ClipBpeTokenizer vs transformers.CLIPTokenizer on a small synthetic vocabulary: equal ids on mixed case, names whose
    underscores became spaces, digits (one token each), an apostrophe, a character outside the vocabulary, a prompt longer than 77
    tokens (truncation keeps EOS last) and ragged lengths (padding with the EOS id)."""
    tf = pytest.importorskip("transformers")
    from concepthash_amd.text import ClipBpeTokenizer
    vocab, merges = ttr.write_tokenizer_files(str(tmp_path))
    ours = ClipBpeTokenizer.from_directory(str(tmp_path))
    theirs = tf.CLIPTokenizer(vocab=vocab, merges=[tuple(m.split()) for m in merges], model_max_length=77)
    ref = theirs(PROMPTS, padding=True, truncation=True, return_tensors="np")["input_ids"]
    got = ours(PROMPTS)
    assert got.dtype == np.int32 and got.shape == ref.shape == (len(PROMPTS), 77)
    assert np.array_equal(got, ref)
    eos = vocab["<|endoftext|>"]
    assert (got[:, 0] == vocab["<|startoftext|>"]).all() and got[6, 76] == eos and (got[3, 6:] == eos).all() and got[3, 4] != eos
    assert vocab["bird</w>"] in got[3] and vocab["10"] not in got[2]       # merges applied; digits split one by one
    short = ours(PROMPTS[:4])
    assert short.shape[1] < 77 and np.array_equal(short, theirs(PROMPTS[:4], padding=True, truncation=True, return_tensors="np")["input_ids"])


def test_tokenizer_product_does_not_import_transformers():
    import os
    from conftest import ROOT
    for rel in ("concepthash_amd/text.py", "trainers/orthohash.py", "concepthash_amd/centers.py"):
        src = open(os.path.join(ROOT, rel)).read()
        assert "import transformers" not in src and "from transformers" not in src, rel


def test_get_codebook_resolves_as_a_target_and_builds_the_plain_codebooks(tmp_path):
    from concepthash_amd.config import instantiate
    for method in ("N", "B"):
        torch.manual_seed(0)
        c = instantiate({"_target_": "trainers.orthohash.get_codebook", "codebook_method": method, "nclass": 7, "nbit": 48})
        assert tuple(c.shape) == (7, 48) and c.dtype == torch.float32 and bool((c.abs() == 1).all())
    from trainers.orthohash import class_prompts, get_codebook
    for method in ("H", "O"):
        with pytest.raises(NotImplementedError, match=f"'{method}'"):
            get_codebook(method, 7, 48)
    names = tmp_path / "class_names.txt"
    names.write_text("001.Black_footed_Albatross\nBrewer_Blackbird \n")
    assert class_prompts(str(names), "a photo of a") == ["a photo of a 001.Black footed Albatross", "a photo of a Brewer Blackbird"]
    with pytest.raises(NotImplementedError, match="quantized"):
        get_codebook("L", 2, 64, class_name_path=str(names), model_id=str(tmp_path), binary_method="pca")
    with pytest.raises(NotImplementedError, match="quantized"):
        get_codebook("L", 2, 64, class_name_path=str(names), model_id=str(tmp_path), quantized=True)
    with pytest.raises(FileNotFoundError, match="hub downloads are not available offline"):
        get_codebook("L", 2, 64, class_name_path=str(names), model_id="openai/clip-vit-base-patch32", quantized=False)


def test_class_centers_without_text_inputs_are_the_seeded_rows(tmp_path):
    """The new keys change nothing for the synthetic datasets and built-in backbone ids: no class_names.txt, or a model id that is no
    local directory with text files -> today's seeded rows."""
    from concepthash_amd.centers import class_centers
    base = class_centers(6, 32, path=str(tmp_path / "none.pt"), seed=4)
    g = torch.Generator().manual_seed(4 + 101)
    assert torch.equal(base, torch.randn(6, 32, generator=g).sign())
    assert torch.equal(base, class_centers(6, 32, path=None, seed=4, class_name_path=str(tmp_path / "class_names.txt"),
                                           model_id="openai/clip-vit-base-patch32"))
    (tmp_path / "class_names.txt").write_text("a\nb\nc\nd\ne\nf\n")
    assert torch.equal(base, class_centers(6, 32, path=None, seed=4, class_name_path=str(tmp_path / "class_names.txt"),
                                           model_id="openai/clip-vit-base-patch32", prompt_prefix="a photo of a "))
    assert torch.equal(base, class_centers(6, 32, path=None, seed=4, class_name_path=str(tmp_path / "class_names.txt"), model_id=str(tmp_path)))


def test_text_config_validation_runs_on_host():
    """ch_text_create checks the config before any device call: no GPU is needed to see the refusals."""
    from concepthash_amd import _lib, build
    build.build()
    lib = _lib.load()
    ok = dict(vocab=64, max_positions=77, dim=128, layers=2, heads=2, ffn=256, act=0, max_batch=4, ln_eps=1e-5)
    t = (_lib.Tensor * 1)()
    for change, word in [(dict(dim=100), b"dim"), (dict(dim=128, heads=4), b"head_dim"), (dict(max_positions=289), b"max_positions"),
                         (dict(max_positions=0), b"max_positions"), (dict(ffn=100), b"ffn"), (dict(act=2), b"act"), (dict(vocab=0), b"vocab"),
                         (dict(max_batch=0), b"max_batch"), (dict(layers=0), b"layers")]:
        h = ctypes.c_void_p()
        bad = _lib.TextConfig(**{**ok, **change})
        assert lib.ch_text_create(ctypes.byref(bad), t, 1, ctypes.byref(h)) != 0, change
        assert word in lib.ch_last_error(), (change, lib.ch_last_error())
        assert not h.value
    assert lib.ch_text_encode(None, None, None, 1, 1, None, None, None) != 0 and b"null handle" in lib.ch_last_error()
    assert lib.ch_text_device_bytes(None) == 0
    lib.ch_text_destroy(None)
