"""Class centres for `LGHWithFixedPrompt(fixed_center=...)`.

The reference builds the (C, 512) centre buffer from CLIP TEXT features of the class names
(trainers/orthohash.py:94-260 `get_codebook`, codebook_method "L").  Here, in this order: a tensor file when `path` exists; the same
language-guided codebook, built by the text tower of the HIP library (trainers/orthohash.py -> concepthash_amd/text.py), when
`class_name_path` exists and `model_id` is a local HF CLIP directory with text weights and tokeniser files; otherwise seeded random
+-1 rows (enough to train and evaluate end to end on synthetic data; a checkpoint's own `center` always overrides it on load)."""
from __future__ import annotations

import logging
import os

import torch


def class_centers(nclass: int, dim: int = 512, path: str = None, seed: int = 0, class_name_path: str = None, model_id=None,
                  prompt_prefix: str = "a photo of a ") -> torch.Tensor:
    def checked(c, what):
        if tuple(c.shape) != (int(nclass), int(dim)):
            raise ValueError(f"{what}: centre tensor has shape {tuple(c.shape)}, expected {(int(nclass), int(dim))}")
        return c

    if path and os.path.exists(str(path)):
        c = torch.load(str(path), map_location="cpu")
        c = c["center"] if isinstance(c, dict) else c
        logging.info("class centres: tensor file %s", path)
        return checked(torch.as_tensor(c, dtype=torch.float32), path)
    if class_name_path and os.path.exists(str(class_name_path)):
        from .text import local_text_files
        if local_text_files(model_id):
            from trainers.orthohash import get_codebook
            c = get_codebook("L", int(nclass), int(dim), class_name_path=str(class_name_path), model_id=model_id,
                             prompt_prefix=prompt_prefix, quantized=False)
            logging.info("class centres: built by the CLIP text tower of %s from %s (%d x %d)", model_id, class_name_path, *c.shape)
            return checked(c, f"text tower of {model_id} on {class_name_path}")
    logging.info("class centres: %s not found -> seeded random +-1 rows (%d x %d)", path, nclass, dim)
    g = torch.Generator().manual_seed(int(seed) + 101)
    return torch.randn(int(nclass), int(dim), generator=g).sign()
