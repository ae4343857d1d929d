"""Plain torch (fp32, CPU) restatement of the CLIP text tower as the language-guided codebook runs it -- shared by
tests/test_text_tower_cpu.py (pinned there against the installed `transformers.CLIPTextModel`) and tests/test_text_tower_gpu.py
(the reference the HIP chain is compared with); not a test itself.

HF `CLIPTextTransformer.forward` with `input_ids` only: token + position embedding, L pre-LN layers whose self-attention is causal
(query t sees keys 0..t; no padding mask), `final_layer_norm` -> last_hidden_state; pooler_output = the row of each prompt's EOS
token: `argmax(ids)` when the config's eos_token_id is 2 (the legacy rule: EOS is the largest id), else the first position
equal to eos_token_id.
"""
from __future__ import annotations

import json
import math
import os

import torch
import torch.nn.functional as F

TM = "text_model."


def eos_positions(ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    ids = ids.to(torch.int64)
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).to(torch.int64).argmax(dim=-1)


def seeded_text_state_dict(dims: dict, seed: int = 0) -> dict:
    """Seeded weights with HF key names.  Linears N(0, 0.5 / sqrt(fan_in)): scores of order one, so the softmax is far from uniform
    and a masking mistake moves the result by much more than any tolerance."""
    g = torch.Generator().manual_seed(seed)
    D, M, L = dims["hidden_size"], dims["intermediate_size"], dims["num_hidden_layers"]

    def n(*shape, std):
        return torch.randn(*shape, generator=g) * std

    sd = {TM + "embeddings.token_embedding.weight": n(dims["vocab_size"], D, std=0.1),
          TM + "embeddings.position_embedding.weight": n(dims["max_position_embeddings"], D, std=0.05)}

    def ln(prefix):
        sd[prefix + ".weight"] = 1.0 + n(D, std=0.1)
        sd[prefix + ".bias"] = n(D, std=0.05)

    def lin(prefix, out_f, in_f):
        sd[prefix + ".weight"] = n(out_f, in_f, std=0.5 / math.sqrt(in_f))
        sd[prefix + ".bias"] = n(out_f, std=0.02)

    for i in range(L):
        pre = TM + f"encoder.layers.{i}."
        for nm in ("k_proj", "v_proj", "q_proj", "out_proj"):
            lin(pre + "self_attn." + nm, D, D)
        ln(pre + "layer_norm1")
        lin(pre + "mlp.fc1", M, D)
        lin(pre + "mlp.fc2", D, M)
        ln(pre + "layer_norm2")
    ln(TM + "final_layer_norm")
    return sd


def text_forward(sd: dict, ids: torch.Tensor, heads: int, act: str = "quick_gelu", eos_token_id: int = 2, eps: float = 1e-5):
    """-> (last_hidden_state [B, T, D], pooler_output [B, D]), fp32, on the device of `ids` (the weights must be there too)"""
    ids = ids.to(torch.int64)
    B, T = ids.shape
    w = {k: v.to(torch.float32) for k, v in sd.items()}
    h = w[TM + "embeddings.token_embedding.weight"][ids] + w[TM + "embeddings.position_embedding.weight"][:T]
    D = h.shape[-1]
    hd = D // heads
    mask = torch.full((T, T), float("-inf"), device=ids.device).triu(1)
    L = 0
    while TM + f"encoder.layers.{L}.layer_norm1.weight" in w:
        L += 1
    for i in range(L):
        pre = TM + f"encoder.layers.{i}."

        def lin(name, x):
            return F.linear(x, w[pre + name + ".weight"], w[pre + name + ".bias"])
        x = F.layer_norm(h, (D,), w[pre + "layer_norm1.weight"], w[pre + "layer_norm1.bias"], eps)
        q, k, v = (lin("self_attn." + nm, x).view(B, T, heads, hd).transpose(1, 2) for nm in ("q_proj", "k_proj", "v_proj"))
        p = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5 + mask, dim=-1)
        h = h + lin("self_attn.out_proj", (p @ v).transpose(1, 2).reshape(B, T, D))
        x = lin("mlp.fc1", F.layer_norm(h, (D,), w[pre + "layer_norm2.weight"], w[pre + "layer_norm2.bias"], eps))
        x = x * torch.sigmoid(1.702 * x) if act == "quick_gelu" else F.gelu(x)
        h = h + lin("mlp.fc2", x)
    hidden = F.layer_norm(h, (D,), w[TM + "final_layer_norm.weight"], w[TM + "final_layer_norm.bias"], eps)
    pooled = hidden[torch.arange(B, device=ids.device), eos_positions(ids, eos_token_id)]
    return hidden, pooled


# ---- a small synthetic CLIP vocabulary: every byte-level character, with and without the end-of-word suffix, a few merges, and the two
# special tokens at the end (as in the real vocabulary, EOS is the largest id)
MERGES = ["a n", "t h", "th e</w>", "o f</w>", "p h", "ph o", "pho t", "phot o</w>", "b i", "bi r", "bir d</w>", "an d</w>",
          "i n", "e r", "' s</w>", "1 0", "in g</w>", "l l", "w a", "wa r", "war b", "b l", "e r</w>"]


def bytes_to_unicode() -> dict:
    """GPT-2's printable stand-ins for the 256 byte values"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def synthetic_vocab(drop: str = "q"):
    """-> (vocab dict, merges list).  The character `drop` is left out of the vocabulary: a word containing it exercises the
    unknown-token path."""
    chars = [c for c in bytes_to_unicode().values() if c != drop]
    tokens = chars + [c + "</w>" for c in chars]
    merges = list(MERGES)
    for m in merges:
        tokens.append(m.replace(" ", ""))
    tokens += ["<|startoftext|>", "<|endoftext|>"]
    return {t: i for i, t in enumerate(tokens)}, merges


def write_tokenizer_files(path: str):
    vocab, merges = synthetic_vocab()
    with open(os.path.join(path, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(os.path.join(path, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(merges) + "\n")
    return vocab, merges


def write_hf_directory(path: str, dims: dict, sd: dict, act: str = "quick_gelu", eos_token_id: int = None, safetensors: bool = True):
    """A local HF CLIP directory: config.json (text_config), the text weights, vocab.json / merges.txt.  dims["vocab_size"] must cover
    the synthetic vocabulary."""
    vocab, _ = write_tokenizer_files(path)
    assert dims["vocab_size"] >= len(vocab)
    eos = vocab["<|endoftext|>"] if eos_token_id is None else eos_token_id
    tc = dict(dims, hidden_act=act, layer_norm_eps=1e-5, eos_token_id=eos, bos_token_id=vocab["<|startoftext|>"], pad_token_id=eos)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "clip", "text_config": tc, "projection_dim": dims["hidden_size"]}, f)
    if safetensors:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    else:
        torch.save(sd, os.path.join(path, "pytorch_model.bin"))
    return vocab
