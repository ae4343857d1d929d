"""GPU: sequences past 288 tokens per image -- the streaming attention kernels (csrc/attention_stream.hip), kernel by kernel against
exact (fp64) attention with the LDS-resident kernels' own error as the yardstick, then the whole encoder at 448 px (ViT-B/16, 789
tokens) and 336 px (ViT-L/14, 581 tokens) against the fp32 oracle, one training step at 294 and 789 tokens against fp32 autograd,
and the proof that nothing changes at or below 288 tokens.  Every measured value is printed (-s).

Bounds.  The streaming forward rounds P to bf16 relative to the RUNNING maximum and multiplies the accumulator by one fp32 rescale
per block: one more rounding of the size the resident kernel already makes, so its error may be at most 2x the resident kernel's --
at the same shape up to 288 tokens, and 2x the resident kernel's error at 288 tokens for every longer sequence.  The same margin
holds for the backward.  The tapped probability rows take the bound tests/test_parity_r2_gpu.py uses at 201 tokens: every entry
within 2e-3 of the exact value, every row sum within 2e-3 of the exact row sum (the rows cover the patch keys only, so the exact
sum is 1 minus the mass on CLS and the concept tokens; with that mass added back the sum must be within 2e-3 of 1)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, load_fixture
from test_train_gpu import _check_grads, _named_grads, _train_model

pytestmark = pytest.mark.gpu

B, H, Q = 2, 3, 4                      # 2 images x 3 heads, 4 concept tokens
RESIDENT, STREAM = 1, 2                # `kernel` of the ch_debug_attention*_ex taps (0 = by length)
LONG = (294, 581, 789, 1029)           # one key past a block edge, ragged tails, the upper limit of the shipped four concept tokens


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import _lib
    return _lib.load()


def _counts(lib):
    return [int(lib.ch_debug_attention_dispatch_count(i)) for i in range(4)]   # fwd resident, fwd streaming, bwd resident, bwd streaming


def _qkv(n, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + n)
    return torch.randn(B * n, 3 * H * 64, generator=g).to(torch.bfloat16).to(dev)


def _split(qkv, n):
    """[B*n, 3*H*64] -> q, k, v as [B, H, n, 64] fp64"""
    t = qkv.double().view(B, n, 3, H, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _exact(qkv, n):
    q, k, v = _split(qkv, n)
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * n, H * 64), p


def _forward(lib, qkv, n, kernel, tap=False, compact=False):
    from concepthash_amd import _lib
    rows = B * (1 + Q) if compact else B * n
    out = torch.zeros(rows, H * 64, dtype=torch.bfloat16, device=qkv.device)
    cattn = torch.full((B, H, Q, n - Q - 1), float("nan"), dtype=torch.float32, device=qkv.device) if tap else None
    _lib.check(lib.ch_debug_attention_ex(_lib.ptr(qkv), B, n, H, _lib.ptr(out), _lib.ptr(cattn), Q, int(compact), kernel,
                                         _lib.stream_ptr()), "ch_debug_attention_ex")
    torch.cuda.synchronize()
    return out, cattn


def _errs(got, ref):
    d = got.double() - ref
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


def _head_rows(n):
    return torch.tensor([b * n + t for b in range(B) for t in [0] + list(range(n - Q, n))])


# ---- 1. forward kernel ----------------------------------------------------------------------------------------------------------
def test_forward_kernel_against_exact_attention(dev, lib):
    """Measured on MI355X (max-abs / RMS error of the bf16 output against fp64 attention on the same bf16 inputs): see DESIGN.md
    section 3.11.  COMPACT rows equal the corresponding rows of the full launch bit for bit, for the resident kernel (201, 288) and
    for the streaming kernel (every length): the per-query arithmetic does not depend on which other queries share the tile."""
    yard = {}
    for n in (201, 288):
        qkv = _qkv(n, dev)
        ref, p = _exact(qkv, n)
        c0 = _counts(lib)
        o_res, _ = _forward(lib, qkv, n, RESIDENT)
        c1 = _counts(lib)
        o_str, tap = _forward(lib, qkv, n, STREAM, tap=True)
        c2 = _counts(lib)
        assert c1[0] - c0[0] == 1 and c1[1] == c0[1] and c2[1] - c1[1] == 1 and c2[0] == c1[0]    # each tap ran the kernel it names
        yard[n] = _errs(o_res, ref)
        e = _errs(o_str, ref)
        print(f"forward {n} tokens: resident max {yard[n][0]:.3e} rms {yard[n][1]:.3e}; streaming max {e[0]:.3e} rms {e[1]:.3e}")
        assert e[0] <= 2 * yard[n][0] and e[1] <= 2 * yard[n][1], (n, e, yard[n])
        _check_tap(tap, p, n)
        o_tap_res, tap_res = _forward(lib, qkv, n, RESIDENT, tap=True)
        assert torch.equal(o_tap_res, o_res)
        print(f"forward {n} tokens: tapped rows, streaming vs resident max diff {float((tap - tap_res).abs().max()):.3e}")
        for kernel, full in ((RESIDENT, o_res), (STREAM, o_str)):
            for with_tap in (False, True):
                oc, tc = _forward(lib, qkv, n, kernel, tap=with_tap, compact=True)
                assert torch.equal(oc.cpu(), full.cpu()[_head_rows(n)]), (n, kernel, with_tap)
                if with_tap:
                    assert torch.equal(tc, tap if kernel == STREAM else tap_res)
    for n in LONG:
        qkv = _qkv(n, dev)
        ref, p = _exact(qkv, n)
        c0 = _counts(lib)
        o, tap = _forward(lib, qkv, n, 0, tap=True)            # by length: must reach the streaming kernel
        c1 = _counts(lib)
        assert c1[1] - c0[1] == 1 and c1[0] == c0[0]
        e = _errs(o, ref)
        print(f"forward {n} tokens: streaming max {e[0]:.3e} rms {e[1]:.3e} (yardstick: resident at 288 tokens)")
        assert e[0] <= 2 * yard[288][0] and e[1] <= 2 * yard[288][1], (n, e, yard[288])
        _check_tap(tap, p, n)
        o_plain, _ = _forward(lib, qkv, n, 0)
        assert torch.equal(o_plain, o)                          # the tap changes nothing in the output
        for with_tap in (False, True):
            oc, tc = _forward(lib, qkv, n, 0, tap=with_tap, compact=True)
            assert torch.equal(oc.cpu(), o.cpu()[_head_rows(n)]), (n, with_tap)
            if with_tap:
                assert torch.equal(tc, tap)


def _check_tap(tap, p, n):
    ref = p[:, :, n - Q:, 1:n - Q]
    rest = p[:, :, n - Q:, :1].sum(-1) + p[:, :, n - Q:, n - Q:].sum(-1)      # exact mass on CLS and the concept tokens
    assert tap.shape == ref.shape and bool(torch.isfinite(tap).all())       # every entry written (the buffer started as NaN)
    d_entry = float((tap.double() - ref).abs().max())
    d_sum = float((tap.double().sum(-1) - ref.sum(-1)).abs().max())
    d_one = float((tap.double().sum(-1) + rest - 1.0).abs().max())
    print(f"tap {n} tokens: entries max diff {d_entry:.3e}, row sums max diff {d_sum:.3e}, |row sum + untapped mass - 1| {d_one:.3e}")
    assert d_entry < 2e-3 and d_sum < 2e-3 and d_one < 2e-3


# ---- 2. backward kernel ---------------------------------------------------------------------------------------------------------
def _exact_bwd(qkv, dO, dpext, n):
    q, k, v = (t.clone().requires_grad_(True) for t in _split(qkv, n))
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * n, H * 64)
    loss = (o * dO.double()).sum()
    if dpext is not None:
        loss = loss + (p[:, :, n - Q:, 1:n - Q] * dpext.double()).sum()
    loss.backward()
    return [t.grad.permute(0, 2, 1, 3).reshape(B * n, H * 64) for t in (q, k, v)]


def _backward(lib, qkv, dO, dpext, n, kernel):
    from concepthash_amd import _lib
    out = torch.full((B * n, 3 * H * 64), float("nan"), dtype=torch.bfloat16, device=qkv.device)
    _lib.check(lib.ch_debug_attention_bwd_ex(_lib.ptr(qkv), _lib.ptr(dO), B, n, H, _lib.ptr(out), _lib.ptr(dpext), Q if dpext is not None else 0,
                                             kernel, _lib.stream_ptr()), "ch_debug_attention_bwd_ex")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ext", [False, True])
def test_backward_kernel_against_exact_attention(dev, lib, ext):
    """dq | dk | dv for a seeded dO, without and with a cotangent on the tapped probability rows (`dpext`, the attention-diversity
    term), against fp64 autograd; the resident backward kernel's error at 201 and 288 tokens is the yardstick (margin 2x, each of dq,
    dk, dv by max-abs and by RMS).  Two runs of the same launch give identical bytes."""
    D = H * 64
    yard = {}

    def case(n):
        qkv = _qkv(n, dev, seed=1)
        g = torch.Generator().manual_seed(7 + n)
        dO = torch.randn(B * n, D, generator=g).to(torch.bfloat16).to(dev)
        dpext = torch.randn(B, H, Q, n - Q - 1, generator=g).to(dev) if ext else None
        return qkv, dO, dpext, _exact_bwd(qkv, dO, dpext, n)

    def errs(got, ref):
        return [_errs(got[:, i * D:(i + 1) * D], ref[i]) for i in range(3)]

    def fmt(e):
        return " ".join(f"{nm} max {a:.3e} rms {r:.3e}" for nm, (a, r) in zip(("dq", "dk", "dv"), e))

    for n in (201, 288):
        qkv, dO, dpext, ref = case(n)
        c0 = _counts(lib)
        g_res = _backward(lib, qkv, dO, dpext, n, RESIDENT)
        c1 = _counts(lib)
        g_str = _backward(lib, qkv, dO, dpext, n, STREAM)
        c2 = _counts(lib)
        assert c1[2] - c0[2] == 1 and c1[3] == c0[3] and c2[3] - c1[3] == 1 and c2[2] == c1[2]
        assert bool(torch.isfinite(g_str.float()).all())        # every element written (the buffer started as NaN)
        yard[n] = errs(g_res, ref)
        e = errs(g_str, ref)
        print(f"backward {n} tokens ext={ext}: resident {fmt(yard[n])}")
        print(f"backward {n} tokens ext={ext}: streaming {fmt(e)}")
        for (a, r), (ya, yr) in zip(e, yard[n]):
            assert a <= 2 * ya and r <= 2 * yr, (n, e, yard[n])
        assert torch.equal(g_str, _backward(lib, qkv, dO, dpext, n, STREAM))
    for n in LONG:
        qkv, dO, dpext, ref = case(n)
        c0 = _counts(lib)
        g_str = _backward(lib, qkv, dO, dpext, n, 0)             # by length: must reach the streaming kernel
        c1 = _counts(lib)
        assert c1[3] - c0[3] == 1 and c1[2] == c0[2]
        assert bool(torch.isfinite(g_str.float()).all())
        e = errs(g_str, ref)
        print(f"backward {n} tokens ext={ext}: streaming {fmt(e)} (yardstick: resident at 288 tokens)")
        for (a, r), (ya, yr) in zip(e, yard[288]):
            assert a <= 2 * ya and r <= 2 * yr, (n, e, yard[288])
        assert torch.equal(g_str, _backward(lib, qkv, dO, dpext, n, 0))


# ---- 3. whole encoder -----------------------------------------------------------------------------------------------------------
def _rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().pow(2).mean().sqrt().clamp_min(1e-12))


def _rms_err(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt() / b.double().pow(2).mean().sqrt().clamp_min(1e-12))


@pytest.mark.parametrize("cfg_name,size,ntok,batch,nbit,nclass", [("vit_b16", 448, 789, 2, 64, 200), ("vit_l14", 336, 581, 1, 128, 555)])
def test_full_depth_encoder_past_288_tokens(dev, lib, cfg_name, size, ntok, batch, nbit, nclass):
    """The seeded oracle weights of the real model sizes evaluated above their pretrain resolution (position table interpolated when
    the engine is built): ViT-B/16 x 12 layers at 448 px, ViT-L/14 x 24 layers at 336 px, against the fp32 oracle on the same
    images.  The project's full-depth bound: 4e-2 max-abs / RMS, 1e-2 RMS / RMS; every sign flip on a code below 4e-2 of the RMS.
    On the parent commit this fails when the model is created (more than 288 tokens per image)."""
    from concepthash_amd.encoder import ConceptHashEncoder
    from oracle import encoder_oracle as eo
    cfg = dict(eo.CONFIGS[cfg_name])
    sd = eo.synthetic_state_dict(cfg, nbit=nbit, nclass=nclass)
    x = eo.synthetic_images(batch, size)
    enc = ConceptHashEncoder(sd, heads=cfg["heads"], max_batch=2, image_size=size)
    assert enc.ntok == ntok
    c0 = _counts(lib)
    out = enc.encode(x.to(dev), want=("codes", "hash_features", "logits_cont", "concept_attn"))
    torch.cuda.synchronize()
    c1 = _counts(lib)
    chains = enc.get_option("last_chains")                       # micro-batch launch chains of that call
    assert c1[1] - c0[1] == cfg["L"] * chains and c1[0] == c0[0]  # every layer's attention ran the streaming kernel
    ref = eo.encode(sd, x, heads=cfg["heads"], with_pooled=False)
    for key in ("codes", "hash_features", "logits_cont"):
        got = out[key].cpu()
        e, r = _rel_err(got, ref[key]), _rms_err(got, ref[key])
        print(f"{cfg_name} x {cfg['L']} layers at {size} px ({ntok} tokens), {key}: vs fp32 oracle max/rms {e:.2e}, rms/rms {r:.2e}")
        assert got.shape == ref[key].shape and e < 4e-2 and r < 1e-2, (key, e, r)
    flips = (out["codes"].cpu() > 0) != (ref["codes"] > 0)
    assert bool((ref["codes"][flips].abs() < 4e-2 * ref["codes"].pow(2).mean().sqrt()).all())
    ca = out["concept_attn"]
    assert ca.shape == (batch, cfg["heads"], 4, ntok - 5) and bool(torch.isfinite(ca).all()) and float(ca.min()) >= 0.0
    h = enc.hidden_states(x.to(dev), 1)                         # ch_encode_hidden at the same size
    assert h.shape[0] == batch and h.shape[1] == ntok and bool(torch.isfinite(h).all())
    enc.close()


# ---- 4. training step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,ntok,attn_div", [(272, 294, 0.0), (448, 789, 0.0), (448, 789, 25.0)])
def test_training_step_past_288_tokens(lib, size, ntok, attn_div):
    """One step of the small training model (train_tiny: D = 128, 2 layers, pretrained at 64 px) on 272 px / 448 px images through the
    drop-in surface against oracle/train_oracle.train_step_grads: the loss and every trainable tensor, by the per-tensor criteria of
    tests/test_train_gpu.py (relative L2 < 4e-2 and cosine > 0.999; the listed small-gradient tensors on the sibling-scaled
    bound).  attn_div = 25: the attention-diversity term on (the probability cotangent of the streaming backward).  A second
    identical step gives an identical gradient arena.

    Inputs.  The head's train-mode BatchNorm divides every code by its standard deviation over the 6 images.  With iid-noise images
    the concept tokens, which average over 289 / 784 iid patches, come out nearly the same for every image: the batch std of the
    pre-BatchNorm codes falls to 4e-4 of their RMS (fp32 oracle; 4.6e-3 for the 64 px fixture step that tests/test_train_gpu.py
    checks) and the smallest |code| to 2e-4 (8e-3 there), so the bf16 forward's 1e-3 differences are amplified tenfold and flip
    binary codes -- at any attention kernel's accuracy.  The images here therefore also differ in colour (a per-image, per-channel
    offset, as photographs do), which restores the fixture's conditioning; the test asserts that on the oracle's own numbers."""
    from models.loss.coop import LGHLoss
    from oracle import encoder_oracle as eo
    from oracle import train_oracle as to
    sd, z = load_fixture("train_tiny")
    model = _train_model(sd, z)
    crit = LGHLoss(margin=0.2, scale=8, loss_scales=dict(logits=0, hash_logits=0, bin_logits=1, cont_logits=1, l2=0, attn_div_loss=attn_div,
                                                         concept_logits=1), avg_before_softmax=False, lmbd=0.5, div_method=1, ncontext=4)
    if attn_div:
        model.return_concept_attention = True
    labels = torch.from_numpy(z["in/labels"])
    colour = 2.0 * torch.randn(labels.shape[0], 3, 1, 1, generator=torch.Generator().manual_seed(11))
    x = (eo.synthetic_images(labels.shape[0], size, seed=11) + colour).to(torch.bfloat16).float()
    c0 = _counts(lib)
    snaps = []
    for _ in range(2):
        model.zero_grad()
        _, out = model(x.cuda())
        loss = crit(out, labels.cuda())
        loss.backward()
        torch.cuda.synchronize()
        snaps.append(model._train_engine.grads.clone())
        if len(snaps) == 1:
            got = _named_grads(model)
    c1 = _counts(lib)
    assert model._train_engine.encoder.ntok == ntok
    assert c1[1] - c0[1] >= 4 and c1[3] - c0[3] >= 4 and c1[0] == c0[0] and c1[2] == c0[2]   # 2 layers x 2 steps, streaming kernels only
    assert torch.equal(snaps[0], snaps[1])
    res = to.train_step_grads(sd, x, labels, heads=int(z["meta/heads"]), upt_heads=8, act=str(z["meta/act"]), attn_div_scale=attn_div)
    v = ((res["out"]["hash_features"] + sd["hash_pe"].float()) @ sd["hash_fc.weight"].float().t()).reshape(labels.shape[0], -1)
    spread = float((v.std(0, unbiased=False) / v.pow(2).mean().sqrt()).min())
    print(f"{ntok} tokens: batch std / RMS of the pre-BatchNorm codes >= {spread:.2e}, smallest |code| {float(res['out']['codes'].abs().min()):.2e}")
    assert spread >= 4.5e-3 and float(res["out"]["codes"].abs().min()) >= 5e-3      # as well conditioned as the 64 px fixture step
    print(f"{ntok} tokens, attn_div {attn_div}: loss {float(loss.detach()):.5f} vs oracle {float(res['loss']):.5f}")
    assert abs(float(loss.detach()) - float(res["loss"])) < (6e-2 if attn_div else 3e-2)
    for k in ("concept", "cont", "bin"):
        assert abs(float(crit.losses[k].detach()) - float(res["losses"][k])) < 2e-2, k
    if attn_div:
        assert abs(float(crit.losses["attn_div"].detach()) - float(res["losses"]["attn_div"])) < 2e-3
        ca = out["concept_attention"].detach().cpu()
        assert float((ca - res["out"]["concept_attention"]).abs().max()) < 2e-3
    # hash_pe adds the same vector to every image's pre-BatchNorm codes: train-mode BatchNorm removes it, with or without the attention
    # term (which does not read it) -- its true gradient is 0 (1.4e-6 in the fp32 oracle), both sides are noise: the floor test applies
    _check_grads(got, res["grads"], floor_keys=("hash_pe",))


# ---- 5. unchanged at and below 288 tokens -----------------------------------------------------------------------------------------
def test_default_dispatch_below_the_limit_is_untouched(dev, lib):
    """201 tokens with default options: the resident kernels run (dispatch counters), and forcing the streaming kernels with the
    model option "attn_stream" and switching it off again leaves no state behind -- the encode outputs and the gradient arena of a
    training step are the bytes they were before."""
    from concepthash_amd.encoder import ConceptHashEncoder
    from oracle import encoder_oracle as eo
    sd, z = load_fixture("encode_n201")
    heads = int(z["meta/heads"])
    x = eo.synthetic_images(2, 224, seed=5).to(torch.bfloat16).float().to(dev)
    want = ("codes", "packed", "logits_cont", "hash_features", "concept_attn")
    enc = ConceptHashEncoder(sd, heads=heads, max_batch=2, options={"streams": 1})      # one launch chain: the counts below are per call
    assert enc.ntok == 201 and enc.get_option("attn_stream") == 0
    c0 = _counts(lib)
    base = {k: v.clone() for k, v in enc.encode(x, want=want).items()}
    torch.cuda.synchronize()
    c1 = _counts(lib)
    assert c1[0] - c0[0] == 2 and c1[1:] == c0[1:]               # 2 layers on the resident kernel, nothing else
    enc.set_option("attn_stream", 1)
    forced = {k: v.clone() for k, v in enc.encode(x, want=want).items()}
    torch.cuda.synchronize()
    c2 = _counts(lib)
    assert c2[1] - c1[1] == 2 and c2[0] == c1[0]
    ref = eo.encode(sd, x.cpu(), heads=heads, with_pooled=False)
    for k in ("codes", "hash_features", "logits_cont"):
        e0, e1 = _rel_err(base[k].cpu(), ref[k]), _rel_err(forced[k].cpu(), ref[k])
        print(f"201 tokens, {k}: resident {e0:.2e}, forced streaming {e1:.2e} vs fp32 oracle")
        assert e1 < 2e-2, k
    assert float((forced["concept_attn"] - base["concept_attn"]).abs().max()) < 2e-3
    enc.set_option("attn_stream", 0)
    again = enc.encode(x, want=want)
    torch.cuda.synchronize()
    c3 = _counts(lib)
    assert c3[0] - c2[0] == 2 and c3[1] == c2[1]
    for k in want:
        assert torch.equal(again[k], base[k]), k
    enc.close()

    # the training step
    model = _train_model(sd, z, 224)
    model.return_concept_attention = True
    cot = torch.randn(2, 4, sd["hash_pe"].shape[-1], generator=torch.Generator().manual_seed(3)).to(dev)
    cot_a = torch.randn(2, heads, 4, 196, generator=torch.Generator().manual_seed(4)).to(dev)

    def step():
        model.zero_grad()
        _, out = model(x)
        torch.autograd.backward([out["hash_features"], out["concept_attention"]], [cot, cot_a])
        torch.cuda.synchronize()
        return model._train_engine.grads.clone(), out["hash_features"].detach().clone()

    c0 = _counts(lib)
    g0, h0 = step()
    c1 = _counts(lib)
    assert c1[0] - c0[0] >= 2 and c1[2] - c0[2] >= 2 and c1[1] == c0[1] and c1[3] == c0[3]
    model._train_engine.encoder.set_option("attn_stream", 1)
    g1, h1 = step()
    c2 = _counts(lib)
    assert c2[1] - c1[1] >= 2 and c2[3] - c1[3] >= 2 and c2[0] == c1[0] and c2[2] == c1[2]
    rel = float((g1 - g0).norm() / g0.norm())
    print(f"201-token training step: gradient arena, forced streaming vs resident relative L2 {rel:.2e}")
    assert rel < 4e-2 and float((h1 - h0).norm() / h0.norm()) < 5e-3
    model._train_engine.encoder.set_option("attn_stream", 0)
    g2, h2 = step()
    assert torch.equal(g2, g0) and torch.equal(h2, h0)


# ---- 6. surface -----------------------------------------------------------------------------------------------------------------
def test_main_v2_evaluates_and_trains_at_a_448_crop(tmp_path):
    """`main_v2.py --config-name val.yaml ... dataset.crop=448` on a run directory from tools/make_synthetic_logdir.py (as
    tests/test_surface_gpu.py does at 224), and a two-batch `exp=hashing` training run at the same crop."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    logdir = str(tmp_path / "run")
    common = ["dataset=synthetic_cub200", "dataset.resize=512", "dataset.crop=448", "data_dir=" + str(tmp_path)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64", "dataset.limit=64"] + common, check=True, env=env,
                   cwd=str(tmp_path))
    ev = str(tmp_path / "ev")
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "--config-name", "val.yaml", "logdir=" + logdir, "batch_size=32",
                    "dataset.limit=64", "save_code=True", "eval_logdir=" + ev] + common, check=True, env=env, cwd=str(tmp_path))
    hist = json.load(open(os.path.join(ev, "history.json")))
    outs = torch.load(os.path.join(ev, "outputs.pth"))
    assert outs["db"]["codes"].shape == (64, 64) and outs["test"]["codes"].shape == (64, 64) and 0.0 < hist["mAP"] <= 1.0
    run2 = str(tmp_path / "train448")
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py"), "exp=hashing", "optim=sgd", "optim.lr=0.02", "scheduler=no_decay",
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64", "epochs=1", "eval_interval=0", "batch_size=16",
                    "dataset.limit=32", "dataset.nclass=8", "logdir=" + run2] + common, check=True, env=env, cwd=str(tmp_path))
    tr = json.load(open(os.path.join(run2, "train_history.json")))
    assert len(tr) == 1 and 0.0 < tr[0]["train_loss"] < 100.0


def test_a_33_by_33_patch_grid_is_refused(dev):
    from concepthash_amd.encoder import ConceptHashEncoder
    sd, z = load_fixture("train_tiny")
    with pytest.raises(RuntimeError, match="32 x 32 patch grid"):
        ConceptHashEncoder(sd, heads=int(z["meta/heads"]), max_batch=1, image_size=33 * 16)
    enc = ConceptHashEncoder(sd, heads=int(z["meta/heads"]), max_batch=1, image_size=32 * 16)   # the limit itself: 1,029 tokens
    assert enc.ntok == 1029
    out = enc.encode(torch.zeros(1, 3, 512, 512, device=dev), want=("codes",))
    assert bool(torch.isfinite(out["codes"]).all())
    enc.close()
