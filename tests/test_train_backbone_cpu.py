"""CPU: the parts of the trainable backbone that need no GPU -- the backbone arena's layout query against the state-dict names and
sizes, the param groups of `backbone_lr_scale`, the separable form of the position-table interpolation (whose transpose carries the
gradient back), and the two optimizer / scheduler config files."""
import os

import pytest
import torch

from concepthash_amd import config as cfglib
from concepthash_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
VM = "backbone.vision_model."


@pytest.mark.parametrize("config", ["vit_b16", "vit_s16", "vit_l14"])
def test_the_arena_layout_query_agrees_with_the_state_dict(config):
    from concepthash_amd.encoder import infer_config
    from concepthash_amd.training import backbone_arena_layout, backbone_arena_names
    cfg = dict(synthetic.CONFIGS[config])
    cfg["L"] = 2 if config != "vit_b16" else cfg["L"]                 # the layout is per layer: two of them show the stride
    sd = synthetic.synthetic_state_dict(cfg, nbit=64, nclass=10, seed=1)
    mc = infer_config(sd, cfg["heads"])
    mc.update(upt_heads=8, act=0, max_batch=1)
    layout = backbone_arena_layout(mc)
    names = backbone_arena_names(cfg["L"])
    # every floating-point tensor of the vision model except the adapters and post_layernorm has a slot, and nothing else has
    want = {k[len(VM):] for k, v in sd.items() if k.startswith(VM) and ".adapt_mlp_" not in k and "post_layernorm" not in k
            and v.is_floating_point()}
    assert set(names) == want
    off = 0
    for name in names:                                                    # contiguous, in the documented order, sizes as the state dict's
        o, n = layout[name]
        assert o == off and n == sd[VM + name].numel(), name
        assert o % 4 == 0, name                                           # the kernels read and write float4s at the slot starts
        off += n
    assert layout["__numel__"][0] == off
    lib_cfg = dict(mc, ln_eps=1e-5, bn_eps=1e-5)
    from concepthash_amd import _lib
    import ctypes
    c = _lib.ModelConfig(**lib_cfg)
    assert _lib.load().ch_backbone_arena_offset(ctypes.byref(c), b"post_layernorm.weight", None) == -1
    assert _lib.load().ch_backbone_arena_offset(ctypes.byref(c), f"encoder.layers.{cfg['L']}.mlp.fc1.bias".encode(), None) == -1


def test_the_position_slot_follows_the_running_resolution():
    from concepthash_amd.training import POS_KEY, backbone_arena_layout
    mc = dict(image_size=448, patch=16, dim=768, layers=1, heads=12, ffn=3072, adapter_dim=384, ncontext=4, nbit=64, nclass=10, proj_dim=512,
              center_dim=512, upt_heads=8, act=0, max_batch=1)
    assert backbone_arena_layout(mc)[POS_KEY][1] == (28 * 28 + 1) * 768


@pytest.mark.parametrize("g,new", [(4, 6), (14, 28), (7, 5)])
def test_the_interpolation_matrix_reproduces_the_table_fold(g, new):
    from concepthash_amd.encoder import interpolate_pos_embedding
    from concepthash_amd.training import pos_interp_matrix
    pos = torch.randn(1 + g * g, 8, generator=torch.Generator().manual_seed(g))
    R = pos_interp_matrix(g, new)
    got = torch.einsum("oy,yxd,px->opd", R, pos[1:].view(g, g, -1).double(), R).reshape(new * new, -1)
    want = interpolate_pos_embedding(pos, new)
    assert torch.allclose(got.float(), want[1:], atol=2e-6, rtol=1e-5)
    # the adjoint used for the gradient is the transpose of the same map: <R x R^T, y> == <x, R^T y R>
    y = torch.randn(new, new, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    x = pos[1:].view(g, g, -1).double()
    lhs = (torch.einsum("oy,yxd,px->opd", R, x, R) * y).sum()
    rhs = (x * torch.einsum("oy,opd,px->yxd", R, y, R)).sum()
    assert abs(float(lhs - rhs)) < 1e-9 * max(1.0, abs(float(lhs)))


class _Model:
    def __init__(self):
        self.bb = torch.nn.Linear(4, 4)
        self.bb.adapter = torch.nn.Linear(2, 2)
        self.head = torch.nn.Linear(4, 2)

    def get_backbone(self):
        return self.bb

    def get_adapter(self):
        return self.bb.adapter

    def get_training_modules(self):
        return self.head


def test_param_groups_follow_the_reference_rule():
    from trainers.base import param_groups
    m = _Model()
    g = param_groups(m, 0.1, 1e-3, True)                    # the whole backbone, adapters included, at scale * lr; then the head
    assert len(g) == 2 and g[0]["lr"] == pytest.approx(1e-4) and "lr" not in g[1]
    assert {id(p) for p in g[0]["params"]} == {id(p) for p in m.bb.parameters()} and len(g[0]["params"]) == 4
    assert {id(p) for p in g[1]["params"]} == {id(p) for p in m.head.parameters()}
    g = param_groups(m, 0, 1e-3, True)                      # frozen backbone: as before
    assert len(g) == 2 and "lr" not in g[0] and {id(p) for p in g[0]["params"]} == {id(p) for p in m.bb.adapter.parameters()}
    g = param_groups(m, 0, 1e-3, False)
    assert len(g) == 1 and {id(p) for p in g[0]["params"]} == {id(p) for p in m.head.parameters()}


def test_the_new_optimizer_and_scheduler_configs_compose(tmp_path):
    cfg = cfglib.compose(CONFIGS, "train.yaml", ["optim=adamw", "scheduler=milestones", "epochs=40", "dataset=synthetic_cub200",
                                                 "backbone_lr_scale=0.1"], cwd=str(tmp_path))
    assert cfg.optim["_target_"] == "torch.optim.adamw.AdamW" and cfg.optim.weight_decay == 0.0 and list(cfg.optim.betas) == [0.9, 0.999]
    assert list(cfg.scheduler.milestones) == [20, 30] and cfg.scheduler.gamma == 0.1 and cfg.backbone_lr_scale == 0.1
    p = [torch.nn.Parameter(torch.zeros(2))]
    opt = cfglib.instantiate(cfg.optim, [{"params": p, "lr": 0.1 * cfg.optim.lr}])
    assert type(opt) is torch.optim.AdamW and opt.param_groups[0]["lr"] == pytest.approx(0.1 * cfg.optim.lr)
    sch = cfglib.instantiate(cfg.scheduler, opt)
    assert type(sch) is torch.optim.lr_scheduler.MultiStepLR


def test_fuse_arena_step_leaves_other_optimizers_alone():
    from concepthash_amd.training import fuse_adapter_sgd, fuse_arena_step
    p = [torch.nn.Parameter(torch.zeros(2))]
    opt = torch.optim.RMSprop(p)
    step = opt.step
    assert fuse_arena_step(opt, object()) is opt and opt.step == step
    adam = torch.optim.Adam(p)
    step = adam.step
    assert fuse_adapter_sgd(adam, object()) is adam and adam.step == step          # the old name still fuses SGD only
    fused = fuse_arena_step(adam, object())                                        # no engine on the model: falls through to torch
    p[0].grad = torch.ones(2)
    fused.step()
    assert fused.fused_adapter_steps["steps"] == 0 and float(p[0].detach().abs().max()) > 0
