"""`trainers.orthohash.get_codebook` / `language_guided_codebook`: the dotted names, parameter names and defaults of the reference's
codebook builders, for what its shipped ConceptHash config calls -- method "L" with `quantized=False`: class names -> prompts ->
CLIP text tower -> `pooler_output` -> sign.  The text tower runs in the HIP library (concepthash_amd/text.py) and `model_id` is a local
HF CLIP directory, not a hub name.  "N" and "B" are the seeded random codebooks; the Hadamard and optimised codebooks and the
quantisers behind `quantized=True` (ITQ, PCA, auto-encoders) are not built here and say so."""
from __future__ import annotations

import logging
import os

import torch

log = logging.getLogger(__name__)
METHODS = ("N", "B", "H", "O", "L")
_NOT_BUILT = {"H": "Hadamard codebook", "O": "optimised codebook"}


def get_codebook(codebook_method, nclass, nbit, **kwargs):
    """(nclass, nbit) of +-1 for "N" (sign of a normal draw) and "B" (fair coin); for "L" the sign of the text features, whose width is
    the text model's, not `nbit`.  One `torch.randn` / `torch.bernoulli` call on the global generator each, so seeded runs repeat."""
    if codebook_method not in METHODS:
        raise ValueError(f"codebook_method must be one of {METHODS}, got {codebook_method!r}")
    if codebook_method in _NOT_BUILT:
        raise NotImplementedError(f"codebook_method '{codebook_method}' ({_NOT_BUILT[codebook_method]}) is not part of the MI355X path")
    if codebook_method == "N":
        return torch.randn(nclass, nbit).sign()
    if codebook_method == "B":
        return torch.bernoulli(torch.full((nclass, nbit), 0.5)).mul(2.0).sub(1.0).sign()
    return centre_rows(language_guided_codebook(nbit=nbit, **kwargs))


def centre_rows(features):
    """The last step of the "L" codebook: text features (`pooler_output`) -> centre rows, their sign (+-1; an exact zero stays 0).  A
    text query (concepthash_amd.text.TextQueryEncoder) turns its own features into a centre row through this function."""
    return features.sign()


def class_prompts(class_name_path, prompt_prefix="a photo of a ", prompt_postfix=""):
    """One class name per line; underscores become spaces, surrounding whitespace goes; a non-empty prefix ends in exactly the space
    that separates it from the name."""
    with open(class_name_path) as f:
        names = [line.replace("_", " ").strip() for line in f]
    prefix = prompt_prefix if not prompt_prefix or prompt_prefix.endswith(" ") else prompt_prefix + " "
    return [f"{prefix}{name}{prompt_postfix}" for name in names]


def language_guided_codebook(class_name_path, nbit, model_id="openai/clip-vit-large-patch14", binary_method="itq", **kwargs):
    """Text features (`pooler_output`, fp32, on the host) of one prompt per class.  `nbit` and `binary_method` only matter to the
    quantisers, which are not built: `quantized` (default True, as in the reference) must be passed as False."""
    if kwargs.get("quantized", True):
        raise NotImplementedError(f"quantized=True (binary_method '{binary_method}': ITQ / PCA / auto-encoder quantisers) is not part of the "
                                  "MI355X path; the shipped config passes quantized=False")
    if not (isinstance(model_id, str) and os.path.isdir(model_id)):
        raise FileNotFoundError(f"CLIP backbone '{model_id}' is not a local directory; hub downloads are not available offline")
    from concepthash_amd.text import ClipBpeTokenizer, TextEncoder

    prompts = class_prompts(class_name_path, kwargs.get("prompt_prefix", "a photo of a "), kwargs.get("prompt_postfix", ""))
    ids = ClipBpeTokenizer.from_directory(model_id)(prompts)
    log.info("language-guided codebook: %d prompts of up to %d tokens, the first one '%s'", len(prompts), ids.shape[1], prompts[0])
    tower = TextEncoder(model_id)
    try:
        features = tower.encode(ids).cpu()
    finally:
        tower.close()
    log.info("language-guided codebook: text features %s from %s", tuple(features.shape), model_id)
    return features
