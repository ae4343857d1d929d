"""Host side of the CLIP text tower (`ch_text_*` in include/concepthash_hip.h): tokeniser, weight loading, encode.

What the reference's language-guided codebook needs (trainers/orthohash.py:94-145): `CLIPProcessor(text=prompts, padding=True,
truncation=True)` -> `CLIPModel.text_model(input_ids).pooler_output`.  PyTorch is used for device memory and file reading only; the
arithmetic runs in the HIP library, and nothing here imports `transformers`.
"""
from __future__ import annotations

import ctypes
import json
import os
import unicodedata
from functools import lru_cache
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import _lib

TM = "text_model."
TEXT_BATCH = 100          # prompts per launch chain: the reference's `text_batch_size = min(nclass, 100)`
_ACTS = {"quick_gelu": 0, "gelu": 1}
_DIM_KEYS = ("vocab_size", "max_position_embeddings", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size")

try:                       # \p{L} / \p{N} need the `regex` module
    import regex as _re
    _SPLIT = _re.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+")
except ImportError:        # the same classes spelled with `re`: letters = word characters that are neither digits nor "_".  Identical on
    import re as _re       # ASCII; `re` counts a few non-decimal numerics (e.g. superscripts) as letters-or-symbols differently
    _SPLIT = _re.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+")
_SPACES = _re.compile(r"\s+")


def eos_positions(ids, eos_token_id: int) -> np.ndarray:
    """Row of every prompt that `pooler_output` reads (transformers 5.15.0 modeling_clip.py:561-581): `argmax(ids)` when the
    config's eos_token_id is 2 (configs older than the fix: EOS is the largest id of the vocabulary), otherwise the FIRST
    position equal to eos_token_id (the padding id may be the same one)."""
    ids = np.asarray(ids, dtype=np.int64)
    if int(eos_token_id) == 2:
        return ids.argmax(axis=-1).astype(np.int32)
    return (ids == int(eos_token_id)).argmax(axis=-1).astype(np.int32)


def _bytes_to_unicode() -> Dict[int, str]:
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


class ClipBpeTokenizer:
    """CLIP's byte-level BPE over a directory's `vocab.json` + `merges.txt`, as `transformers.CLIPTokenizer` applies it without
    `ftfy`: NFC, whitespace runs -> one space, lower case, CLIP's split pattern, bytes -> printable stand-ins, merges by rank with
    `</w>` on the last symbol of a word, BOS / EOS added, truncated to `max_length` (EOS kept), padded to the longest prompt."""

    BOS, EOS = "<|startoftext|>", "<|endoftext|>"

    def __init__(self, vocab: Dict[str, int], merges: Iterable[str], max_length: int = 77, pad_token: Optional[str] = None):
        self.vocab = dict(vocab)
        pairs = [tuple(m.split()) for m in merges if m.strip() and not m.startswith("#version")]
        self.ranks = {p: i for i, p in enumerate(pairs)}
        self.byte_chars = _bytes_to_unicode()
        self.bos_id, self.eos_id = self.vocab[self.BOS], self.vocab[self.EOS]
        self.unk_id = self.eos_id                                   # CLIPTokenizer: unk_token = "<|endoftext|>"
        self.pad_id = self.vocab[pad_token] if pad_token else self.eos_id
        self.max_length = int(max_length)
        self._word = lru_cache(maxsize=65536)(self._bpe)

    @classmethod
    def from_directory(cls, path: str) -> "ClipBpeTokenizer":
        with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
        with open(os.path.join(path, "merges.txt"), encoding="utf-8") as f:
            merges = f.read().split("\n")
        max_length, pad = 77, None
        cfg = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(cfg):
            with open(cfg) as f:
                tc = json.load(f)
            ml = tc.get("model_max_length", 77)
            max_length = int(ml) if isinstance(ml, (int, float)) and 0 < ml <= 4096 else 77
            p = tc.get("pad_token")
            p = p.get("content") if isinstance(p, dict) else p
            pad = p if p in vocab else None
        return cls(vocab, merges, max_length=max_length, pad_token=pad)

    def _bpe(self, word: str) -> tuple:
        sym = list(word[:-1]) + [word[-1] + "</w>"]
        while len(sym) > 1:
            best = min(zip(sym, sym[1:]), key=lambda p: self.ranks.get(p, 1 << 60))
            if best not in self.ranks:
                break
            out, i = [], 0
            while i < len(sym):
                if i + 1 < len(sym) and (sym[i], sym[i + 1]) == best:
                    out.append(sym[i] + sym[i + 1])
                    i += 2
                else:
                    out.append(sym[i])
                    i += 1
            sym = out
        return tuple(self.vocab.get(s, self.unk_id) for s in sym)

    def encode(self, text: str) -> List[int]:
        text = _SPACES.sub(" ", unicodedata.normalize("NFC", text)).lower()
        ids = [self.bos_id]
        for piece in _SPLIT.findall(text):
            if piece == self.BOS or piece == self.EOS:
                ids.append(self.vocab[piece])
                continue
            ids.extend(self._word("".join(self.byte_chars[b] for b in piece.encode("utf-8"))))
        ids.append(self.eos_id)
        if len(ids) > self.max_length:
            ids = ids[:self.max_length - 1] + [self.eos_id]
        return ids

    def __call__(self, prompts: Iterable[str]) -> np.ndarray:
        """-> int32 [len(prompts), longest], padded with the pad id"""
        rows = [self.encode(p) for p in prompts]
        T = max(len(r) for r in rows)
        out = np.full((len(rows), T), self.pad_id, dtype=np.int32)
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
        return out


def local_text_files(model_id) -> bool:
    """True when `model_id` is a local HF CLIP directory that holds what the text tower needs: config, weights, tokeniser files"""
    if not isinstance(model_id, str) or not os.path.isdir(model_id):
        return False
    have = lambda *names: any(os.path.exists(os.path.join(model_id, n)) for n in names)   # noqa: E731
    return have("config.json") and have("model.safetensors", "pytorch_model.bin") and have("vocab.json") and have("merges.txt")


class TextEncoder:
    """CLIP text tower on one MI355X, through the C-ABI.  `source`: a local HF CLIP directory (`config.json` with `text_config`,
    `model.safetensors` / `pytorch_model.bin` -- the files models/backbone/clip.py reads the vision half from), or a dict of
    text_config dimensions together with `state_dict` (keys `text_model.*`)."""

    def __init__(self, source, state_dict: Optional[Dict[str, torch.Tensor]] = None, max_batch: int = TEXT_BATCH,
                 device: Optional[torch.device] = None):
        self.lib = _lib.load()
        if isinstance(source, dict):
            if state_dict is None:
                raise ValueError("TextEncoder(dims) needs the state_dict as well")
            tc = dict(source)
        else:
            if not (isinstance(source, str) and os.path.isdir(source)):
                raise FileNotFoundError(f"CLIP text model '{source}' is not a local directory; hub downloads are not available offline")
            with open(os.path.join(source, "config.json")) as f:
                cfg = json.load(f)
            tc = dict(cfg.get("text_config") or cfg)
            st = os.path.join(source, "model.safetensors")
            if os.path.exists(st):
                from safetensors.torch import load_file
                state_dict = load_file(st)
            else:
                state_dict = torch.load(os.path.join(source, "pytorch_model.bin"), map_location="cpu")
        missing = [k for k in _DIM_KEYS if k not in tc]
        if missing:
            raise KeyError(f"text_config lacks {missing}")
        act = tc.get("hidden_act", "quick_gelu")
        if act not in _ACTS:
            raise ValueError(f"text tower activation '{act}' is not supported (quick_gelu, gelu)")
        self.eos_token_id = int(tc.get("eos_token_id", 2))
        self.dim, self.max_positions, self.vocab = int(tc["hidden_size"]), int(tc["max_position_embeddings"]), int(tc["vocab_size"])
        self.max_batch = int(max_batch)
        c = _lib.TextConfig(vocab=self.vocab, max_positions=self.max_positions, dim=self.dim, layers=int(tc["num_hidden_layers"]),
                            heads=int(tc["num_attention_heads"]), ffn=int(tc["intermediate_size"]), act=_ACTS[act],
                            max_batch=self.max_batch, ln_eps=float(tc.get("layer_norm_eps", 1e-5)))
        keep, entries = [], []
        for k, v in state_dict.items():
            if not k.startswith(TM) or k.endswith("position_ids") or not torch.is_tensor(v):
                continue
            t = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            entries.append((k.encode(), t))
        if not entries:
            raise KeyError("no `text_model.*` tensors: the checkpoint holds no CLIP text tower")
        arr = (_lib.Tensor * len(entries))()
        for i, (name, t) in enumerate(entries):
            arr[i].name = name
            arr[i].data = ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))
            arr[i].numel = t.numel()
        handle = ctypes.c_void_p()
        self._h = None
        if not torch.cuda.is_available():
            raise RuntimeError("TextEncoder needs a GPU (MI355X); there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ch_text_create(ctypes.byref(c), arr, len(entries), ctypes.byref(handle)), "ch_text_create")
        self._h = handle

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ch_text_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        return int(self.lib.ch_text_device_bytes(self._h))

    def encode_batch(self, ids: np.ndarray, eos: np.ndarray, want_hidden: bool = False):
        """One `ch_text_encode` call: ids int32 [B, T] and eos int32 [B] on the host -> pooled [B, D] (and hidden [B, T, D]) on the device"""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        eos = np.ascontiguousarray(eos, dtype=np.int32)
        B, T = ids.shape
        with torch.cuda.device(self.device):
            pooled = torch.empty(B, self.dim, dtype=torch.float32, device=self.device)
            hidden = torch.empty(B, T, self.dim, dtype=torch.float32, device=self.device) if want_hidden else None
            i32p = ctypes.POINTER(ctypes.c_int32)
            _lib.check(self.lib.ch_text_encode(self._h, ids.ctypes.data_as(i32p), eos.ctypes.data_as(i32p), B, T, _lib.ptr(pooled),
                                               _lib.ptr(hidden), _lib.stream_ptr()), "ch_text_encode")
        return pooled, hidden

    def encode(self, ids, want_hidden: bool = False):
        """ids [N, T] (any integer array / tensor) -> pooler_output [N, D] fp32 on the device (, last_hidden_state [N, T, D]); prompts
        go through in batches of at most `max_batch` (100: the reference's text batch)."""
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids)
        if ids.ndim != 2 or ids.shape[0] == 0:
            raise ValueError(f"ids must be [N, T] with N >= 1, got {ids.shape}")
        eos = eos_positions(ids, self.eos_token_id)
        pooled, hidden = [], []
        for i in range(0, ids.shape[0], self.max_batch):
            p, h = self.encode_batch(ids[i:i + self.max_batch], eos[i:i + self.max_batch], want_hidden)
            pooled.append(p)
            hidden.append(h)
        pooled = torch.cat(pooled, dim=0)
        return (pooled, torch.cat(hidden, dim=0)) if want_hidden else pooled


DEFAULT_PREFIX = "a photo of a "          # configs/model/*.yaml `model.fixed_center.prompt_prefix`, as the reference's codebook builder has it


def _cfg(node, *path, default=None):
    for key in path:
        if node is None or not hasattr(node, "get"):
            return default
        node = node.get(key)
    return default if node is None else node


def text_query_settings(config, text_model=None, prefix=None):
    """(text model directory, prompt prefix) of a run for text queries, from its config alone -- no model is built and no GPU touched.
    `text_model` / `prefix` override `model.backbone.name` / `model.fixed_center.prompt_prefix` ("" = no prefix).  One ValueError names
    everything that is missing: a local HF CLIP directory with text weights and tokeniser files, a model with `text_projection`."""
    source = text_model if text_model is not None else _cfg(config, "model", "backbone", "name")
    missing = []
    if not local_text_files(source):
        missing.append(f"'{source}' ({'text_model' if text_model is not None else 'model.backbone.name'}) is not a local HF CLIP directory "
                       "with config.json, model.safetensors / pytorch_model.bin, vocab.json and merges.txt")
    target = str(_cfg(config, "model", "_target_", default=""))
    if not target.endswith("LGHWithFixedPrompt"):
        missing.append(f"the model ({target or 'no model._target_'}) has no text_projection: only LGHWithFixedPrompt maps text features "
                       "onto the code space")
    if missing:
        raise ValueError("text queries are not possible for this run: " + "; ".join(missing))
    if prefix is None:
        prefix = _cfg(config, "model", "fixed_center", "prompt_prefix", default=DEFAULT_PREFIX)
    return str(source), str(prefix)


class TextQueryEncoder:
    """Prompt strings -> query codes of a run ("text query"): tokenise `prefix + prompt`, `pooler_output` of the
    text tower, the centre row the "L" codebook makes of it (`trainers.orthohash.centre_rows`), and the model's own `text_projection`
    through `ch_model_project_text`.  Owns the tower's handle: `close()` (or the `with` block) releases it."""

    def __init__(self, model, text_model, prefix: str = DEFAULT_PREFIX, max_batch: int = TEXT_BATCH, device=None):
        missing = []
        if not local_text_files(text_model):
            missing.append(f"'{text_model}' is not a local HF CLIP directory with config.json, model.safetensors / pytorch_model.bin, "
                           "vocab.json and merges.txt")
        if getattr(model, "text_projection", None) is None or not hasattr(model, "project_text"):
            missing.append(f"the model ({type(model).__name__}) has no text_projection")
        if missing:
            raise ValueError("text queries are not possible: " + "; ".join(missing))
        self.model, self.text_model, self.prefix = model, str(text_model), str(prefix)
        self.tokenizer = ClipBpeTokenizer.from_directory(self.text_model)
        self.tower = TextEncoder(self.text_model, max_batch=max_batch, device=device if device is not None else model.center.device)
        cd = int(model.center.shape[1])
        if self.tower.dim != cd:
            self.close()
            raise ValueError(f"the text tower of '{text_model}' is {self.tower.dim} wide, the model's centres are {cd} wide: not the text "
                             "model this run's centres were built with")

    def close(self):
        tower, self.tower = getattr(self, "tower", None), None
        if tower is not None:
            tower.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def prompts(self, prompts, prefix: Optional[str] = None) -> List[str]:
        prompts = [prompts] if isinstance(prompts, str) else [str(p) for p in prompts]
        if not prompts:
            raise ValueError("no prompt given")
        prefix = self.prefix if prefix is None else str(prefix)
        return [prefix + p for p in prompts]

    def features(self, ids) -> torch.Tensor:
        """ids [N, T] -> pooler_output [N, Dt] on the device, in the tower's batches of at most `max_batch` prompts"""
        return self.tower.encode(ids)

    def project(self, features: torch.Tensor) -> torch.Tensor:
        from trainers.orthohash import centre_rows
        return self.model.project_text(centre_rows(features))

    def text_codes(self, prompts, prefix: Optional[str] = None) -> torch.Tensor:
        """-> [N, nbit] fp32 on the device: real-valued query codes, used exactly as an image's pre-sign codes"""
        return self.project(self.features(self.tokenizer(self.prompts(prompts, prefix))))

    def center_agreement(self, class_name_path: str, prefix: Optional[str] = None) -> float:
        """Share of equal entries between the centres this tower rebuilds from `class_name_path` and the model's `center` buffer: 1.0
        when the tower, the tokeniser and the prefix are the ones the run's centres came from.  A class count other than the model's is
        refused; anything else is reported (a warning below 1), never judged."""
        import logging
        from trainers.orthohash import centre_rows, class_prompts
        prompts = class_prompts(class_name_path, self.prefix if prefix is None else str(prefix))
        center = self.model.center.detach()
        if len(prompts) != center.shape[0]:
            raise ValueError(f"{class_name_path} names {len(prompts)} classes, the model's centres have {center.shape[0]} rows")
        rebuilt = centre_rows(self.features(self.tokenizer(prompts)))
        share = float((rebuilt == center.to(rebuilt.device)).float().mean())
        if share < 1.0:
            logging.warning("text queries: %.4f of the centre entries rebuilt from %s by the text tower of %s equal the checkpoint's `center` "
                            "buffer; the run's centres were built with another text model, tokeniser or prompt prefix", share,
                            class_name_path, self.text_model)
        return share
