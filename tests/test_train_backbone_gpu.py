"""GPU: the trainable backbone (`backbone_lr_scale != 0`) -- every encoder weight's gradient out of the HIP backward, against fp32
autograd of oracle/train_oracle.py (the graph that tests/golden/train_tiny.npz pins to the reference) with `requires_grad` on the
backbone keys; the fused Adam / AdamW / SGD arena step; the trainer end to end.

Acceptance of one gradient tensor: the rule of tests/test_train_gpu.py -- relative L2 error < 4e-2 and cosine > 0.999.  A tensor named
in CANCELLED_SUM_TENSORS may instead pass on an absolute error below 3e-2 of the largest gradient norm of its ROLE (the same tensor
in the other layers; for k_proj.bias the role of q_proj.bias).  No 2-D weight matrix is on that list.  Figures: run with -s.
"""
import pytest
import torch

from conftest import fixture_images, load_fixture
from test_surface_cpu import _model_like_fixture

pytestmark = pytest.mark.gpu
VM = "backbone.vision_model."

# Tensors that may take the role-scaled absolute bound, each with its reason; a figure is the worst abs error / role norm seen.
CANCELLED_SUM_TENSORS = {
    # softmax is invariant to a shift common to all keys: the exact gradient is ZERO, what the kernel returns is the bf16 noise of a
    # column sum of dK.  Compared against q_proj.bias's scale.
    # Measured: 2.7e-3 of q_proj.bias's norm at worst (train_tiny), 2.1e-3 at full depth.
    "self_attn.k_proj.bias": "exact gradient 0 (softmax shift invariance)",
    # the adapters' own list (tests/test_train_gpu.py SMALL_GRADIENT_TENSORS)
    ".adapt_mlp_2.": "second adapter: gradient ~1/27 of the first's",
    ".adapt_mlp_1.scale": "scalar sum over every row and column",
}
MATRIX_SUFFIXES = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "out_proj.weight", "fc1.weight", "fc2.weight", "patch_embedding.weight")


def _role(k):
    import re
    if ".adapt_mlp_" in k:
        return k.split(".adapt_mlp_")[1][2:]
    r = re.sub(r"encoder\.layers\.\d+\.", "", k)
    return r.replace("k_proj.bias", "q_proj.bias")


def _backbone_keys(sd):
    return [k for k in sd if k.startswith(VM) and ".adapt_mlp_" not in k and "post_layernorm" not in k and "position_ids" not in k
            and sd[k].is_floating_point()]


def _check(got, want, label=""):
    scale, worst_role = {}, {}
    for k, ref in want.items():
        scale[_role(k)] = max(scale.get(_role(k), 0.0), float(ref.double().norm()))
    failures = []
    for k, ref in want.items():
        assert k in got, f"no gradient for {k}"
        g, r = got[k].double().flatten(), ref.double().flatten()
        err = float((g - r).norm())
        rel = err / max(float(r.norm()), 1e-30)
        cos = float(torch.dot(g, r) / (g.norm() * r.norm()).clamp_min(1e-30))
        role = _role(k)
        if rel < 4e-2 and cos > 0.999:
            worst_role[role] = max(worst_role.get(role, 0.0), rel)
            continue
        listed = any(t in k for t in CANCELLED_SUM_TENSORS) and not k.endswith(MATRIX_SUFFIXES)
        a = err / max(scale[role], 1e-30)
        print(f"{label} BOUND {k}: rel {rel:.3e} cos {cos:.5f} abs/role {a:.3e} own/role {float(r.norm()) / max(scale[role], 1e-30):.3e}")
        if not listed:
            failures.append((k, rel, cos, a))
        elif a >= 3e-2:
            failures.append((k, rel, cos, a))
    for role in sorted(worst_role):
        print(f"{label} worst relative L2 error, {role}: {worst_role[role]:.3e}")
    assert not failures, failures


def _colour_images(n, size, seed):
    """Images that also differ in colour (a per-image, per-channel offset, as tests/test_long_sequence_gpu.py): over near-identical
    samples the head's train-mode BatchNorm makes every sum over rows cancel, and bf16 noise is then measured against almost nothing."""
    from oracle import encoder_oracle as eo
    colour = 2.0 * torch.randn(n, 3, 1, 1, generator=torch.Generator().manual_seed(seed))
    return (eo.synthetic_images(n, size, seed=seed) + colour).to(torch.bfloat16).float()


def _train_model(sd, z, image_size=64, backbone=True):
    model = _model_like_fixture(z, sd, image_size)
    model.load_state_dict(sd)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.hash_attention.sa.dropout = 0.0
    model = model.cuda()
    model.train()
    if backbone:
        model.get_backbone().requires_grad_(True)
    return model


def _named_grads(model):
    return {k: p.grad.detach().float().cpu() for k, p in model.named_parameters(remove_duplicate=False)
            if not k.startswith(("adapter_params.", "trainable_params.")) and p.grad is not None}


def _oracle_loss_grads(sd, x, labels, heads, act, keys, attn_scale):
    from oracle import train_oracle as to
    sdg = {k: v.clone() for k, v in sd.items()}
    for k in keys:
        sdg[k] = sdg[k].float().requires_grad_(True)
    out = to.forward_train(sdg, x, heads=heads, upt_heads=8, act=act)
    loss = sum(to.margin_ce(out[n], labels, 8.0, 0.2) for n in ("logits_concept", "logits_cont", "logits_bin"))
    loss = loss + attn_scale * to.attn_div(out["concept_attention"], 1)
    loss.backward()
    return float(loss.detach()), {k: sdg[k].grad.detach() for k in keys}


def _cancellation(sd, z, x, labels):
    """kappa = sqrt(sum_r |g_r|^2) / |sum_r g_r| of the MLP bias gradients, on the CPU oracle: the biases are expanded to one copy per
    token row, so that autograd returns every row's term g_r of the sum."""
    from oracle import train_oracle as to
    sdg = {k: v.clone() for k, v in sd.items()}
    B, N = x.shape[0], 1 + (x.shape[-1] // sd[VM + "embeddings.patch_embedding.weight"].shape[-1]) ** 2 + 4
    keys = [VM + f"encoder.layers.{l}.mlp.{f}.bias" for l in range(2) for f in ("fc1", "fc2")]
    for k in keys:
        sdg[k] = sdg[k].float().expand(B, N, -1).clone().requires_grad_(True)
    out = to.forward_train(sdg, x, heads=int(z["meta/heads"]), upt_heads=8, act=str(z["meta/act"]))
    loss = sum(to.margin_ce(out[n], labels, 8.0, 0.2) for n in ("logits_concept", "logits_cont", "logits_bin"))
    (loss + 25.0 * to.attn_div(out["concept_attention"], 1)).backward()
    res = {}
    for k in keys:
        g = sdg[k].grad.reshape(B * N, -1).double()
        res[k[len(VM) + 15:]] = round(float(g.pow(2).sum().sqrt() / g.sum(0).norm()), 2)
    return res


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("chains", [1, 2])
@pytest.mark.parametrize("name,size,batch", [("train_tiny", 64, 12), ("encode_n201", 224, 12)])
def test_every_backbone_gradient_through_the_loss(name, size, batch, chains, prune, monkeypatch):
    """The train_tiny architecture at 21 tokens and the 201-token fixture (D = 256), through `LGHWithFixedPrompt.train()`, `LGHLoss` with the
    attention-diversity term on (its cotangent enters the attention backward), `loss.backward()`: every backbone tensor, and the adapters.

    Choice of the batch, made on the CPU oracle alone (`_cancellation`).  The head's train-mode BatchNorm makes the cotangents of the
    concept rows sum to zero over the batch, and the residual path carries that sum unchanged down the layers; what enters fc2 / fc1 /
    layer_norm2 is only that stream (plus the small second adapter), so their gradients are sums over rows that cancel by a factor kappa
    = sqrt(sum_r |g_r|^2) / |sum_r g_r|.  The forward's bf16 error (3e-3 of a row, tests/test_train_gpu.py `_vjp_against_oracle`) comes
    back through the BatchNorm into every row's cotangent and does NOT cancel, so the floor under such a tensor is about 3e-3 * kappa.
    With twelve images of twelve classes kappa is 58 / 62 (fc2.bias, layer 0 / 1) at 21 tokens and 26 / 30 at 201 -- measured there on
    MI355X: fc1 / fc2.weight 6.4e-2 .. 8.0e-2 and 4.1e-2 .. 4.4e-2, their biases up to 1.6e-1, error orthogonal to the gradient, the
    attention side (kappa 6) inside the rule.  With the twelve images in ONE class kappa is 3.2 .. 3.4 and 2.1 .. 2.2: every weight matrix
    then has a gradient well above that floor (3e-3 * 3.4 = 1e-2), and that is the batch used.  The test asserts kappa < 8 before it compares."""
    from models.loss.coop import LGHLoss
    from oracle import train_oracle as to
    monkeypatch.setenv("CH_TRAIN_STREAMS", str(chains))
    monkeypatch.setenv("CH_TRAIN_CHAIN_MIN_ROWS", "1")
    monkeypatch.setenv("CH_TRAIN_PRUNE_LAST", str(prune))
    sd, z = load_fixture(name)
    x = _colour_images(batch, size, seed=11)
    labels = torch.zeros(batch, dtype=torch.long)          # one class: see the docstring
    kappa = _cancellation(sd, z, x, labels)
    print("cancellation factors:", kappa)
    assert max(kappa.values()) < 8, kappa
    model = _train_model(sd, z, size)
    model.return_concept_attention = True
    crit = LGHLoss(margin=0.2, scale=8, loss_scales=dict(logits=0, hash_logits=0, bin_logits=1, cont_logits=1, l2=0, attn_div_loss=25,
                                                         concept_logits=1), avg_before_softmax=False, lmbd=0.5, div_method=1, ncontext=4)
    _, out = model(x.cuda())
    loss = crit(out, labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    keys = _backbone_keys(sd) + [k for k in to.trainable_keys(sd) if ".adapt_mlp_" in k]
    ref_loss, want = _oracle_loss_grads(sd, x, labels, int(z["meta/heads"]), str(z["meta/act"]), keys, 25.0)
    print(f"loss {float(loss.detach()):.5f} oracle {ref_loss:.5f}")
    assert abs(float(loss.detach()) - ref_loss) < 6e-2
    for k in (VM + "encoder.layers.0.mlp.fc1.weight", VM + "embeddings.patch_embedding.weight"):     # well above the bf16 noise floor
        assert float(want[k].norm()) > 1e-4, (k, float(want[k].norm()))
    assert model.backbone.vision_model.post_layernorm.weight.grad is None        # as in the reference: no loss term reads it
    _check(_named_grads(model), want, f"{name}/chains{chains}/prune{prune}")


def test_a_coherent_cotangent_pins_the_mlp_weight_gradients():
    """The same cotangent vector on every concept row of every image (as test_vjp_with_a_coherent_cotangent_pins_the_last_adapter): the
    sums over rows behind fc1 / fc2 / layer_norm2 add up coherently, so these tensors are measured against a gradient that is not a
    cancelled sum, whatever the images are."""
    from oracle import train_oracle as to
    sd, z = load_fixture("train_tiny")
    x = fixture_images(z)
    model = _train_model(sd, z)
    cot = torch.randn(1, 1, sd["hash_pe"].shape[-1], generator=torch.Generator().manual_seed(5)).expand(x.shape[0], 4, -1).contiguous()
    model(x.cuda())[1]["hash_features"].backward(cot.cuda())
    torch.cuda.synchronize()
    keys = _backbone_keys(sd)
    sdg = {k: v.clone() for k, v in sd.items()}
    for k in keys:
        sdg[k] = sdg[k].float().requires_grad_(True)
    to.forward_train(sdg, x, heads=int(z["meta/heads"]), upt_heads=8, act=str(z["meta/act"]))["hash_features"].backward(cot)
    _check(_named_grads(model), {k: sdg[k].grad for k in keys}, "train_tiny/coherent")


def _vjp_on_model(model, x, cot, cot_attn=None):
    """model side of a VJP test: hash_features' cotangent `cot`, optionally every layer's concept-attention rows' `cot_attn`"""
    _, out = model(x.cuda())
    obj = (out["hash_features"] * cot.cuda()).sum()
    if cot_attn is not None:
        obj = obj + (out["concept_attention_layers"] * cot_attn.cuda()).sum()
    obj.backward()
    torch.cuda.synchronize()
    return out


def _vjp_on_oracle(sd, z, x, cot, keys, cot_attn=None):
    from oracle import train_oracle as to
    sdg = {k: v.clone() for k, v in sd.items()}
    for k in keys:
        sdg[k] = sdg[k].float().requires_grad_(True)
    out = to.forward_train(sdg, x, heads=int(z["meta/heads"]), upt_heads=8, act=str(z["meta/act"]))
    obj = (out["hash_features"] * cot).sum()
    if cot_attn is not None:
        obj = obj + (out["concept_attention_layers"] * cot_attn).sum()
    obj.backward()
    return out, {k: sdg[k].grad.detach() for k in keys}


def test_after_the_weights_moved_everything_follows_the_arena():
    """Every other comparison runs at the initial weights, where the arena equals the model's frozen copy -- a kernel that still read the
    frozen copy would pass them all.  Here every backbone tensor is moved first (5 % of its mean magnitude, kept bf16-representable as the
    fixture's weights are), the engine re-derives its working copies, and `hash_features`, the gradients that flow through
    d(concept tokens) (hash_queries, hash_attention.*: they pass pre_layrnorm's gamma) and every backbone gradient are compared with the
    oracle on the UPDATED state dict.  A second pass does the same after a fused Adam step."""
    from concepthash_amd.training import fuse_arena_step
    from oracle import train_oracle as to
    sd, z = load_fixture("train_tiny")
    x = fixture_images(z)
    model = _train_model(sd, z)
    model.get_training_modules().requires_grad_(True)
    cot = torch.randn(1, 1, sd["hash_pe"].shape[-1], generator=torch.Generator().manual_seed(5)).expand(x.shape[0], 4, -1).contiguous()
    _vjp_on_model(model, x, cot)                                  # builds the engine: the parameters are arena views from here on
    eng = model._train_engine
    gen = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for p in eng.backbone_parameters():
            noise = torch.randn(p.shape, generator=gen).cuda() * 0.05 * p.abs().mean()
            p.copy_((p + noise).to(torch.bfloat16).float())
    groups = [{"params": list(model.get_backbone().parameters())}, {"params": list(model.get_training_modules().parameters())}]
    opt = fuse_arena_step(torch.optim.Adam(groups, lr=2e-3), model)
    for label in ("moved", "moved+adam"):
        model.zero_grad()
        out = _vjp_on_model(model, x, cot)
        now = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        sd_now = {k: now.get(k, v) for k, v in sd.items()}
        assert not torch.equal(sd_now[VM + "pre_layrnorm.weight"], sd[VM + "pre_layrnorm.weight"])
        keys = _backbone_keys(sd) + ["hash_queries"] + [k for k in to.trainable_keys(sd) if k.startswith("hash_attention.")]
        ref, want = _vjp_on_oracle(sd_now, z, x, cot, keys)
        rel = float((out["hash_features"].detach().cpu() - ref["hash_features"].detach()).norm() / ref["hash_features"].detach().norm())
        print(f"{label}: hash_features relative error {rel:.3e}")
        assert rel < 1e-2, rel
        _check(_named_grads(model), want, "train_tiny/" + label)
        if label == "moved":
            opt.step()
            assert opt.fused_adapter_steps["steps"] == 1


def test_every_layers_attention_cotangent_reaches_the_backbone():
    """The second concept-attention layout (`return_concept_attention = "all"`, the `avg_attn` form): a cotangent on every layer's rows
    [L, B, heads, Q, Np] next to the one on hash_features, every backbone tensor against the oracle."""
    sd, z = load_fixture("train_tiny")
    x = fixture_images(z)
    model = _train_model(sd, z)
    model.return_concept_attention = "all"
    g = torch.Generator().manual_seed(6)
    cot = torch.randn(1, 1, sd["hash_pe"].shape[-1], generator=g).expand(x.shape[0], 4, -1).contiguous()
    cot_attn = torch.randn(2, x.shape[0], int(z["meta/heads"]), 4, 16, generator=g)
    out = _vjp_on_model(model, x, cot, cot_attn)
    assert tuple(out["concept_attention_layers"].shape) == tuple(cot_attn.shape)
    keys = _backbone_keys(sd)
    _, want = _vjp_on_oracle(sd, z, x, cot, keys, cot_attn)
    _check(_named_grads(model), want, "train_tiny/all-layers")


def test_unbatched_reductions_give_the_same_bytes():
    """`train_batched_grads` 0 and 1 (it batches the adapters' reductions only; the backbone's products reduce inline under either): both
    gradient arenas byte-identical, with two chains and the every-layer attention cotangent."""
    from concepthash_amd.training import TrainEngine, adapters_from_state_dict, backbone_from_state_dict
    sd, z = load_fixture("train_tiny")
    x = fixture_images(z).cuda()
    D = sd["hash_pe"].shape[-1]
    b = sd[VM + "encoder.layers.0.adapt_mlp_1.down_proj.weight"].shape[0]
    g = torch.Generator().manual_seed(8)
    ctx = (torch.randn(4, D, generator=g) * 0.5).cuda()
    cot = torch.randn(x.shape[0], 4, D, generator=g).cuda()
    cot_attn = torch.randn(2, x.shape[0], int(z["meta/heads"]), 4, 16, generator=g).cuda()
    snaps = []
    for batched in (1, 0):
        eng = TrainEngine(sd, adapters_from_state_dict(sd, 2, D, b), heads=int(z["meta/heads"]), act=str(z["meta/act"]), max_batch=x.shape[0],
                          device=x.device, backbone=backbone_from_state_dict(sd),
                          options={"train_batched_grads": batched, "train_chains": 2, "train_chain_min_rows": 1})
        eng.forward(x, ctx, want_attn="all")
        dct = eng.backward(cot, cot_attn)
        torch.cuda.synchronize()
        snaps.append((eng.bgrads.clone(), eng.grads.clone(), dct.clone()))
        eng.close()
    assert float(snaps[0][0].abs().max()) > 0
    for a, c in zip(snaps[0], snaps[1]):
        assert torch.equal(a, c)


def _full_model(cfg, sd):
    from concepthash_amd import config as cfglib
    from models.arch.coop import LGHWithFixedPrompt
    from models.backbone.clip import CLIP
    dims = dict(hidden_size=cfg["D"], num_hidden_layers=cfg["L"], num_attention_heads=cfg["heads"], intermediate_size=cfg["M"],
                patch_size=cfg["patch"], image_size=cfg["image"], projection_dim=cfg["P"], hidden_act="quick_gelu")
    upt = cfglib.DictConfig(multi=True, num_heads=8, dropout=0.0, ensemble_method="concat", single_hash_fc=True, hash_pe=True)
    C, cd = sd["center"].shape
    nbit = sd["hash_fc.weight"].shape[0] * 4
    tp = torch.nn.Sequential(torch.nn.Linear(cd, cd), torch.nn.ReLU(), torch.nn.Linear(cd, nbit))
    model = LGHWithFixedPrompt(CLIP(dims, allow_random_init=True), nbit, C, 4, add_bn=True, upt_config=upt, fixed_center=torch.zeros(C, cd),
                               text_projection=tp, has_adapter=True, adapter_bottleneck_dim=cfg["b"], concept_reg=True)
    model.load_state_dict(sd)
    model = model.cuda().train()
    model.get_backbone().requires_grad_(True)
    return model


def _vjp_case(cfg, size, batch, seed, label):
    """d(hash_features) = a random cotangent through the public surface against fp32 autograd of the oracle on the CPU"""
    from concepthash_amd import synthetic
    from oracle import train_oracle as to
    sd = synthetic.synthetic_state_dict(cfg, nbit=64, nclass=10, seed=3)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    model = _full_model(cfg, sd)
    x = _colour_images(batch, size, seed)
    cot = torch.randn(batch, 4, cfg["D"], generator=torch.Generator().manual_seed(seed))
    _, out = model(x.cuda())
    out["hash_features"].backward(cot.cuda())
    torch.cuda.synchronize()
    keys = _backbone_keys(sd)
    sdg = {k: v.clone() for k, v in sd.items()}
    for k in keys:
        sdg[k] = sdg[k].float().requires_grad_(True)
    hf = to.forward_train(sdg, x, heads=cfg["heads"])["hash_features"]
    hf.backward(cot)
    rel = float((out["hash_features"].detach().cpu() - hf.detach()).norm() / hf.detach().norm())
    print(f"{label} hash_features relative error {rel:.3e}")
    assert rel < 1e-2, rel
    want = {k: sdg[k].grad.detach() for k in keys}
    for k in keys:
        if k.endswith(MATRIX_SUFFIXES):
            assert float(want[k].norm()) > 1e-5, (k, float(want[k].norm()))
    _check(_named_grads(model), want, label)
    return model


def test_full_depth_vit_b16_every_backbone_gradient():
    """ViT-B/16 x 12 layers on the seeded weights, three images: every backbone tensor against the oracle's fp32 autograd."""
    from concepthash_amd import synthetic
    _vjp_case(dict(synthetic.CONFIGS["vit_b16"]), 224, 3, 5, "vit_b16x12")


def test_streaming_attention_and_the_interpolated_position_table():
    """448 px = 789 tokens of ViT-B/16 (two layers): the streaming attention kernels, and the gradient of the PRETRAIN-size position table
    through the adjoint of the bicubic interpolation (the oracle differentiates F.interpolate)."""
    from concepthash_amd import synthetic
    cfg = dict(synthetic.CONFIGS["vit_b16"])
    cfg["L"] = 2
    model = _vjp_case(cfg, 448, 2, 7, "vit_b16x2@448")
    pos = model.backbone.vision_model.embeddings.position_embedding.weight
    assert tuple(pos.shape) == (197, 768) and tuple(pos.grad.shape) == (197, 768)


@pytest.mark.parametrize("chains", [1, 2])
def test_backbone_gradients_are_byte_identical_run_to_run(chains, monkeypatch):
    monkeypatch.setenv("CH_TRAIN_STREAMS", str(chains))
    monkeypatch.setenv("CH_TRAIN_CHAIN_MIN_ROWS", "1")
    sd, z = load_fixture("encode_n201")
    model = _train_model(sd, z, 224)
    x = _colour_images(4, 224, 2).cuda()
    cot = torch.randn(4, 4, sd["hash_pe"].shape[-1], generator=torch.Generator().manual_seed(2)).cuda()
    snaps = []
    for _ in range(2):
        model.zero_grad()
        model(x)[1]["hash_features"].backward(cot)
        torch.cuda.synchronize()
        eng = model._train_engine
        snaps.append((eng.bgrads.clone(), eng.grads.clone()))
    assert float(snaps[0][0].abs().max()) > 0
    assert torch.equal(snaps[0][0], snaps[1][0]) and torch.equal(snaps[0][1], snaps[1][1])


# ch_trainer_bytes of a frozen-backbone trainer, ViT-B/16 (12 layers), max_batch 32, default options: measured on the parent commit and on
# this one (the same number: the backbone path allocates nothing for a trainer created by ch_trainer_create)
FROZEN_TRAINER_BYTES_B16_BATCH32 = 3571860576     # parent commit: 3,571,860,576; this commit: 3,571,860,576 (trainable backbone: more)


def test_a_frozen_trainer_allocates_and_computes_nothing_new():
    from concepthash_amd import synthetic
    from concepthash_amd.training import TrainEngine, adapters_from_state_dict, backbone_from_state_dict
    cfg = dict(synthetic.CONFIGS["vit_b16"])
    sd = synthetic.synthetic_state_dict(cfg, nbit=64, nclass=10, seed=3)
    dev = torch.device("cuda", torch.cuda.current_device())
    eng = TrainEngine(sd, adapters_from_state_dict(sd, cfg["L"], cfg["D"], cfg["b"]), heads=cfg["heads"], max_batch=32, device=dev)
    frozen = int(eng.lib.ch_trainer_bytes(eng._t))
    assert eng.bparams is None and eng.bgrads is None and eng._bviews == []
    eng.close()
    eng = TrainEngine(sd, adapters_from_state_dict(sd, cfg["L"], cfg["D"], cfg["b"]), heads=cfg["heads"], max_batch=32, device=dev,
                      backbone=backbone_from_state_dict(sd))
    trainable = int(eng.lib.ch_trainer_bytes(eng._t))
    eng.close()
    print(f"ch_trainer_bytes ViT-B/16 batch 32: frozen {frozen}, trainable backbone {trainable}")
    assert frozen == FROZEN_TRAINER_BYTES_B16_BATCH32
    assert trainable > frozen


def _adam_reference(p, g, m, v, step, lr, b1, b2, eps, wd, decoupled):
    """float64 restatement of torch.optim.Adam / AdamW, single tensor, amsgrad False"""
    if decoupled:
        p = p * (1 - lr * wd)
    elif wd:
        g = g + wd * p
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    return p - lr / (1 - b1 ** step) * m / denom, m, v


@pytest.mark.parametrize("cls", ["Adam", "AdamW"])
def test_adam_step_against_torch_and_float64(cls):
    """ch_adam_step over a flat array against torch.optim.Adam / AdamW (foreach=False) on the same device, five steps with weight decay:
    its distance from a float64 restatement is at most twice torch's own, plus one ulp of the parameter."""
    from concepthash_amd import _lib
    lib = _lib.load()
    n = 1 << 16
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g).cuda()
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 5e-2
    pt = torch.nn.Parameter(p0.clone())
    opt = getattr(torch.optim, cls)([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    pf, m, v = p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pr, mr, vr = p0.double(), torch.zeros(n, device="cuda", dtype=torch.float64), torch.zeros(n, device="cuda", dtype=torch.float64)
    for step in range(1, 6):
        grad = (torch.randn(n, generator=g) * 0.1).cuda()
        pt.grad = grad.clone()
        opt.step()
        _lib.check(lib.ch_adam_step(_lib.ptr(pf), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), n, lr, b1, b2, eps, wd, int(cls == "AdamW"), step,
                                    _lib.stream_ptr()), "ch_adam_step")
        pr, mr, vr = _adam_reference(pr, grad.double(), mr, vr, step, lr, b1, b2, eps, wd, cls == "AdamW")
        torch.cuda.synchronize()
        d_torch = float((pt.detach().double() - pr).abs().max())
        d_fused = float((pf.double() - pr).abs().max())
        ulp = float(torch.finfo(torch.float32).eps * pr.abs().max())
        print(f"{cls} step {step}: |torch - f64| {d_torch:.3e}  |fused - f64| {d_fused:.3e}  ulp {ulp:.3e}")
        assert d_fused <= 2 * d_torch + ulp, (step, d_fused, d_torch)


@pytest.mark.parametrize("cls", ["Adam", "AdamW", "SGD"])
def test_the_fused_arena_step_over_both_arenas(cls):
    """`fuse_arena_step` with group 0 = the whole backbone: both arenas stepped by one launch each, against a float64 restatement (bound as
    above, torch's own distance taken from a plain-torch twin); group 1 is stepped by torch and equals the twin bit for bit.  The gradients
    are seeded tensors written into the `.grad`s, the same in both runs, so that the two runs see identical inputs at every step."""
    from concepthash_amd.training import fuse_arena_step
    sd, z = load_fixture("train_tiny")
    x = fixture_images(z).cuda()
    kw = dict(lr=1e-2, weight_decay=5e-2)
    if cls == "SGD":
        kw["momentum"] = 0.9
    runs = []
    for fused in (False, True):
        model = _train_model(sd, z)
        model(x)[1]["hash_features"].sum().backward()          # builds the engine; the parameters are arena views from here on
        groups = [{"params": list(model.get_backbone().parameters()), "lr": 1e-3},
                  {"params": list(model.get_training_modules().parameters())}]
        opt = getattr(torch.optim, cls)(groups, foreach=False, **kw)
        if fused:
            opt = fuse_arena_step(opt, model)
        eng = model._train_engine
        start = (eng.params.double().clone(), eng.bparams.double().clone())
        gen = torch.Generator().manual_seed(9)
        grads_seen = []
        for step in range(4):
            ga = (torch.randn(eng.grads.shape, generator=gen) * 0.1).cuda()
            gb = (torch.randn(eng.bgrads.shape, generator=gen) * 0.1).cuda()
            eng.grads.copy_(ga)
            eng.bgrads.copy_(gb)
            for p, gv in eng._views + eng._bviews:
                p.grad = gv
            for p in groups[1]["params"]:
                p.grad = (torch.randn(p.shape, generator=gen) * 0.1).cuda()
            grads_seen.append((ga.double(), gb.double()))
            opt.step()
        torch.cuda.synchronize()
        if fused:
            assert opt.fused_adapter_steps["steps"] == 4
        runs.append((model, eng, start, grads_seen))
    (m0, e0, start, seen), (m1, e1, _, _) = runs
    for idx, name in ((0, "adapter"), (1, "backbone")):
        p = start[idx]
        m, v, buf = torch.zeros_like(p), torch.zeros_like(p), None
        for step, gs in enumerate(seen, 1):
            g = gs[idx]
            if cls == "SGD":
                d = g + kw["weight_decay"] * p
                buf = d.clone() if buf is None else 0.9 * buf + d
                p = p - 1e-3 * buf
            else:
                p, m, v = _adam_reference(p, g, m, v, step, 1e-3, 0.9, 0.999, 1e-8, kw["weight_decay"], cls == "AdamW")
        torch_p = (e0.params, e0.bparams)[idx].double()
        fused_p = (e1.params, e1.bparams)[idx].double()
        d_torch, d_fused = float((torch_p - p).abs().max()), float((fused_p - p).abs().max())
        ulp = float(torch.finfo(torch.float32).eps * p.abs().max())
        print(f"{cls} {name} arena: |torch - f64| {d_torch:.3e}  |fused - f64| {d_fused:.3e}  ulp {ulp:.3e}")
        assert d_fused <= 2 * d_torch + ulp, (name, d_fused, d_torch)
    a, b = dict(m0.get_training_modules().named_parameters()), dict(m1.get_training_modules().named_parameters())
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_main_v2_trains_the_backbone_end_to_end(optim, tmp_path):
    """`main_v2.py ... backbone_lr_scale=0.1 epochs=2`: the loss falls, a backbone weight has moved, the evaluation that follows and a
    re-evaluation of the saved checkpoint give the same score (the checkpoint holds the moved weights and reloads to the same codes)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    logdir = str(tmp_path / "run")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["dataset=synthetic_cub200", "dataset.limit=128", "dataset.nclass=8", "data_dir=" + str(tmp_path)]
    lr = {"adam": "optim.lr=0.001", "sgd": "optim.lr=0.02"}[optim]
    base = [sys.executable, os.path.join(ROOT, "main_v2.py"), "exp=hashing", "optim=" + optim, lr, "scheduler=no_decay",
            "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64", "batch_size=32", "backbone_lr_scale=0.1"]
    subprocess.run(base + ["epochs=2", "eval_interval=2", "logdir=" + logdir] + common, check=True, env=env, cwd=str(tmp_path))
    tr = json.load(open(os.path.join(logdir, "train_history.json")))
    te = json.load(open(os.path.join(logdir, "test_history.json")))
    assert len(tr) == 2 and tr[-1]["train_loss"] < tr[0]["train_loss"], [t["train_loss"] for t in tr]
    assert abs(tr[0]["lr/0"] - 0.1 * tr[0]["lr/1"]) < 1e-12
    ck = torch.load(os.path.join(logdir, "models/last.pth"), map_location="cpu")
    from models.backbone.clip import CLIP
    fresh = CLIP("synthetic/clip-vit-small-patch16", allow_random_init=True).model.vision_model.state_dict()
    key = "encoder.layers.5.mlp.fc1.weight"
    moved = float((ck[VM + key] - fresh[key]).abs().max())
    print(f"{optim}: losses {[t['train_loss'] for t in tr]}, max |delta| of {key}: {moved:.3e}")
    assert moved > 1e-6
    ev = str(tmp_path / "ev")
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "--config-name", "val.yaml", "logdir=" + logdir, "batch_size=32",
                    "eval_logdir=" + ev] + common, check=True, env=env, cwd=str(tmp_path))
    hist = json.load(open(os.path.join(ev, "history.json")))
    assert abs(hist["mAP"] - te[0]["mAP"]) < 1e-12
    if optim == "adam":
        r = subprocess.run(base + ["epochs=1", "model.has_adapter=False", "logdir=" + str(tmp_path / "noad")] + common, env=env,
                           cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode != 0 and "NotImplementedError" in r.stderr
