"""Plain fp64 restatements of the CLIP text tower's own two kernels (text_model.hip: text_embed_kernel, text_pool_kernel), each with its
DERIVED bound, an fp32 emulation with switchable deliberate defects, and `compose`: one text layer's stages in Hugging Face order, each
stage delegated to the reference and bound its launcher already has (forward_kernels_ref.layernorm_ref, gemm_ref.out_ref / resid_ref,
attention_ref.bounds).  Shared by tests/test_text_chain_ref_cpu.py (CPU) and tests/test_text_chain_gpu.py (GPU); not a test itself.
Nothing is tuned to a measured error.  The vocabulary (U32, gam, two_pass, ln_affine, rsqrt_err, TINY, row_family, ROW_FAMILIES) is that of
tests/train_kernels_ref.py and tests/forward_kernels_ref.py.

text_embed_kernel: H[row] = tok[ids[row]] + pos[row % T], ONE fp32 addition of two fp32 table entries (commutative, correctly rounded):
the comparison is bit for bit and carries no bound.

text_pool_kernel: out[r] = LayerNorm(H[src(r)]) with fp32 rows in and out; src(r) = r * T + eos[r] in eos mode, r otherwise.  The kernel
is the two-pass form of rowops.hip's row_stats / row_affine, restated in its own file: a lane adds x + y of each of its D / 128 float2
pairs into its sum (one rounding for the pair, D / 128 for the chain), then wave_sum's six xor steps: n = 1 + D / 128 + 6 additions on the
longest path of one row reduction = forward_kernels_ref.n_row_stats(D) (read off text_model.hip; the squares a a + c c take the place of
x + y, the two extra roundings of two_pass are the square and the division by D).  The affine step recomputes v - mean and rounds three
more times ((c rstd) w + b: ln_affine).  The output stays fp32, so there is no bf16 term: the bound is a few u32 of the row's magnitude
and a result that went through bf16 anywhere (2^-9 relative) leaves it by four orders of magnitude.  rsqrtf keeps the 2^-22 of rsqrt_err.
"""
import torch

import attention_ref as ar
import forward_kernels_ref as fr
import gemm_ref as gr
from train_kernels_ref import ROW_FAMILIES, TINY, U32, bits_equal, breaches, f32, gam, gen as _tr_gen, row_family, rsqrt_err  # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16
TM = "text_model."
VOCAB = 64

# ---- the cases of tests/test_text_chain_gpu.py; tests/test_text_chain_ref_cpu.py walks the same ones ----------------------------------
EMBED_D = (128, 384, 1280)
EMBED_BT = ((1, 1), (3, 5), (2, 77), (1, 288))               # 1, 15, 154 and 288 rows: three of them no multiple of the 4 rows per workgroup
EMBED_POS_EXTRA = 3                                          # the position table holds T + 3 rows: pos[row] is not pos[row % T] from B = 2 on
EMBED_DEFECTS = ("pos_of_row", "tok_of_neighbour")
POOL_D = (128, 384, 768, 1280)
POOL_ROWS = (1, 5, 37)
POOL_EPS = (1e-5, 1e-6)
POOL_EOS = ((5, 7, (0, 6, 3, 6, 0)), (1, 1, (0,)))           # (B, T, eos)
POOL_MAX_POSITIONS = 9                                       # what `eos_stride_max_positions` strides by where T = 7
POOL_DEFECTS = ("eos_plus_1", "eos_stride_max_positions", "pool_through_bf16") + fr.LN_DEFECTS


def gen(name, *key):
    return _tr_gen("text_chain/" + name, *key)


# ---- text_embed_kernel ------------------------------------------------------------------------------------------------------------------
def embed_inputs(B, T, D):
    """(ids [B * T] int32 holding 0 and 63 (63 alone where there is one row), tok [VOCAB, D], pos [T + EMBED_POS_EXTRA, D]); neighbouring
    rows of either table are unrelated, so a row taken one off is a different row"""
    g = gen("embed", B, T, D)
    ids = torch.randint(0, VOCAB, (B * T,), generator=g).to(torch.int32)
    ids[0], ids[-1] = 0, VOCAB - 1
    return ids, torch.randn(VOCAB, D, generator=g), torch.randn(T + EMBED_POS_EXTRA, D, generator=g)


def embed_ref(ids, T, tok, pos):
    """H [rows, D] fp32, exact: one correctly rounded addition"""
    rows = ids.numel()
    return tok[ids.long()] + pos[torch.arange(rows) % T]


def embed_emul(ids, T, tok, pos, defect=None):
    """the kernel's index arithmetic row by row, the operands of the addition the other way round"""
    rows = ids.numel()
    r = torch.arange(rows)
    t = r.clamp_max(pos.shape[0] - 1) if defect == "pos_of_row" else r % T
    src = ids.long()[(r + 1) % rows] if defect == "tok_of_neighbour" else ids.long()
    return pos[t] + tok[src]


# ---- text_pool_kernel -------------------------------------------------------------------------------------------------------------------
def pool_rows(H, eos, T, defect=None, max_positions=None):
    """the rows of H the kernel normalises (defective gathers stay inside H, as a test must)"""
    if eos is None:
        return H
    r = torch.arange(eos.numel())
    e = eos.long() + (1 if defect == "eos_plus_1" else 0)
    src = r * (max_positions if defect == "eos_stride_max_positions" else T) + e
    return H[src % H.shape[0]]


def pool_ref(H, eos, T, w, b, eps):
    """(out, bound) fp64: two-pass LayerNorm of fp32 rows, fp32 output; n = n_row_stats(D) (module docstring); row r reads
    H[r * T + eos[r]] with eos, H[r] without"""
    x = pool_rows(H, eos, T).double()
    c, R, e_c, e_r = fr.two_pass(x, fr.n_row_stats(x.shape[1]), f32(eps))
    return fr.ln_affine(c, R, e_c, e_r, w.double(), b.double())


def pool_emul(H, eos, T, w, b, eps, defect=None, max_positions=POOL_MAX_POSITIONS):
    """fp32 with torch's reductions (another order than the kernel's)"""
    y = fr.ln_f32(pool_rows(H, eos, T, defect, max_positions), w, b, eps, defect if defect in fr.LN_DEFECTS else None)
    return y.to(BF16).float() if defect == "pool_through_bf16" else y


# ---- one text layer, stage by stage ------------------------------------------------------------------------------------------------------
STAGES = ("ln1", "qkv", "attn", "out_proj", "ln2", "fc1", "fc2")
ACT_EPI = {"quick_gelu": gr.EPI_QUICK, "gelu": gr.EPI_GELU}


def layer_weights(sd, i):
    """Layer i of a state dict with Hugging Face names, as the loader holds it: fp32 LayerNorm tables and biases, the four GEMM weights
    rounded to bf16 (round to nearest even).  The fused q | k | v weight [3D, D] and bias [3D] are stacked HERE from the three separate
    projections: rows 0 .. D - 1 are q_proj's, then k_proj's, then v_proj's (the column blocks attention_ref.split reads)."""
    pre = TM + f"encoder.layers.{i}."
    g = lambda n: sd[pre + n].detach().to("cpu", F32)   # noqa: E731
    proj = ("q_proj", "k_proj", "v_proj")
    return dict(ln1_w=g("layer_norm1.weight"), ln1_b=g("layer_norm1.bias"), ln2_w=g("layer_norm2.weight"), ln2_b=g("layer_norm2.bias"),
                qkv_w=torch.cat([g(f"self_attn.{p}.weight") for p in proj], 0).to(BF16),
                qkv_b=torch.cat([g(f"self_attn.{p}.bias") for p in proj], 0),
                out_w=g("self_attn.out_proj.weight").to(BF16), out_b=g("self_attn.out_proj.bias"),
                fc1_w=g("mlp.fc1.weight").to(BF16), fc1_b=g("mlp.fc1.bias"), fc2_w=g("mlp.fc2.weight").to(BF16), fc2_b=g("mlp.fc2.bias"))


def compose(stage, w, x, B, T, heads, act="quick_gelu", eps=1e-5, h=None):
    """(want, bound), fp64, of ONE stage of a CLIP text layer (transformers CLIPEncoderLayer with a causal mask and no padding mask, as
    tests/text_tower_ref.text_forward restates it) from that stage's input x [B * T, .] and, for the two residual additions, the
    residual stream h [B * T, D] it adds to:
        ln1       x = h fp32             -> layer_norm1(h)                                  bf16
        qkv       x = ln1's output bf16  -> q_proj | k_proj | v_proj (x) + bias             bf16 [., 3D]
        attn      x = qkv's output       -> softmax(q k^T / 8, keys <= query) v per head     bf16
        out_proj  x = attn's output, h   -> h + out_proj(x)                                  fp32 (the new residual stream)
        ln2       x = h fp32             -> layer_norm2(h)                                  bf16
        fc1       x = ln2's output       -> act(fc1(x)), act = quick_gelu or exact gelu      bf16 [., ffn]
        fc2       x = fc1's output, h    -> h + fc2(x)                                       fp32
    `out_proj_copy` / `fc2_copy`: the bf16 copy of the projection itself (out_proj(x), fc2(x)) that the residual epilogue also stores.
    Every bound is the launcher's own: layernorm_ref with n_row_stats(D), gemm_ref's epilogues 0, 1 / 2 and 3, attention_ref's causal one."""
    if stage in ("ln1", "ln2"):
        return fr.layernorm_ref(x, w[stage + "_w"], w[stage + "_b"], fr.n_row_stats(x.shape[1]), eps)
    if stage == "qkv":
        return gr.out_ref(gr.EPI_BIAS, gr.Ops(x, w["qkv_w"], w["qkv_b"]))
    if stage == "attn":
        out, bound, _, _ = ar.bounds(x, B, T, heads, causal=True)
        return out, bound
    if stage == "fc1":
        return gr.out_ref(ACT_EPI[act], gr.Ops(x, w["fc1_w"], w["fc1_b"]))
    name, copy = (stage[:-5], True) if stage.endswith("_copy") else (stage, False)
    if name in ("out_proj", "fc2"):
        o = gr.Ops(x, w[("out" if name == "out_proj" else "fc2") + "_w"], w[("out" if name == "out_proj" else "fc2") + "_b"], h=h)
        return gr.out_ref(gr.EPI_BIAS_RESID, o) if copy else gr.resid_ref(gr.EPI_BIAS_RESID, o)
    raise KeyError(stage)


def compose_forward(sd, ids, heads, layers, act="quick_gelu", eps=1e-5):
    """The whole tower through `compose` in fp64 with NO intermediate rounding (every stage's `want` is the next stage's input), weights
    as layer_weights holds them: last_hidden_state [B, T, D] fp64.  What the CPU test holds against text_tower_ref.text_forward."""
    B, T = ids.shape
    flat = ids.reshape(-1).to(torch.int32)
    h = embed_ref(flat, T, sd[TM + "embeddings.token_embedding.weight"].float(), sd[TM + "embeddings.position_embedding.weight"].float()).double()
    for i in range(layers):
        w = layer_weights(sd, i)
        x = h
        for stage in STAGES:
            x = compose(stage, w, x, B, T, heads, act, eps, h=h)[0]
            if stage in ("out_proj", "fc2"):
                h = x
    out, _ = pool_ref(h, None, T, sd[TM + "final_layer_norm.weight"].float(), sd[TM + "final_layer_norm.bias"].float(), eps)
    return out.view(B, T, -1)
