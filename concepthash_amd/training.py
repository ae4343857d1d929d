"""Training step of the ConceptHash adapters on the MI355X HIP library (C-ABI `ch_trainer_*` / `ch_train_*`,
include/concepthash_hip.h).

What runs where (reference: trainers/coop.py:107-131 `train_one_batch`):
  * HIP library: the encoder forward with saved activations and its backward -- everything on the [B*N, *] activations, the
    gradients of the 24 adapters' parameters, and the gradient w.r.t. the concept tokens;
  * this module: the parameter plumbing.  The adapters' parameters live in ONE fp32 device arena (the layout
    `ch_adapter_arena_numel` describes); the `nn.Parameter`s of the adapter modules are re-pointed at views of it, their
    `.grad`s at views of the gradient arena the library overwrites, so an ordinary optimizer updates the arena in place and
    `refresh()` re-derives the library's bf16 / folded / transposed working copies;
  * the caller's autograd: the 4-token concept generator, the hashing head on [B, Q, D] and the loss (models/arch/coop.py,
    models/loss/coop.py) -- a few MFLOP per step -- joined to the library by `EncoderFunction`.

There is no CPU fallback: without the HIP library (or without a GPU) construction raises.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence

import torch

from . import _lib
from .encoder import VM, ConceptHashEncoder

ADAPTER_FIELDS = ("adapter_layer_norm.weight", "adapter_layer_norm.bias", "down_proj.weight", "down_proj.bias", "up_proj.weight",
                  "up_proj.bias", "scale")


# the backbone arena (include/concepthash_hip.h): per encoder layer, then the embedding side; names below `vision_model.`
BACKBONE_LAYER_FIELDS = ("layer_norm1.weight", "layer_norm1.bias", "self_attn.q_proj.weight", "self_attn.q_proj.bias", "self_attn.k_proj.weight",
                         "self_attn.k_proj.bias", "self_attn.v_proj.weight", "self_attn.v_proj.bias", "self_attn.out_proj.weight",
                         "self_attn.out_proj.bias", "layer_norm2.weight", "layer_norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                         "mlp.fc2.bias")
BACKBONE_EMBED_FIELDS = ("embeddings.class_embedding", "embeddings.patch_embedding.weight", "embeddings.position_embedding.weight",
                         "pre_layrnorm.weight", "pre_layrnorm.bias")
POS_KEY = "embeddings.position_embedding.weight"


def backbone_arena_names(layers: int) -> List[str]:
    """State-dict names (below `vision_model.`) of the backbone arena's tensors, in arena order.  `post_layernorm` is not among them: no
    term of the training loss reads it (reference models/arch/coop.py:498-501 feeds `image_features`, which models/loss/coop.py never
    touches), so its gradient is None there and here."""
    return [f"encoder.layers.{l}.{f}" for l in range(layers) for f in BACKBONE_LAYER_FIELDS] + list(BACKBONE_EMBED_FIELDS)


def backbone_arena_layout(cfg: dict) -> Dict[str, tuple]:
    """name -> (offset, numel) in floats, asked of the library (`ch_backbone_arena_offset`; needs no GPU).  cfg: the model dimensions
    (`encoder.infer_config` keys; image_size = the resolution the engine runs at)."""
    lib = _lib.load()
    fields = {n for n, _ in _lib.ModelConfig._fields_}
    c = _lib.ModelConfig(**{k: v for k, v in cfg.items() if k in fields})
    out = {}
    for name in backbone_arena_names(cfg["layers"]):
        numel = ctypes.c_int64()
        off = int(lib.ch_backbone_arena_offset(ctypes.byref(c), name.encode(), ctypes.byref(numel)))
        if off < 0:
            raise RuntimeError(f"the library has no backbone arena slot for {name}")
        out[name] = (off, int(numel.value))
    out["__numel__"] = (int(lib.ch_backbone_arena_numel(ctypes.byref(c))), 0)
    return out


def pos_interp_matrix(g: int, new_grid: int) -> torch.Tensor:
    """R [new_grid, g] with interpolate_pos_embedding(pos)[1:] = R grid R^T per channel (the bicubic resize is separable and linear; clamped
    tap indices accumulate).  Its transpose is the adjoint that carries the gradient of the interpolated table back to the parameter."""
    import math

    import numpy as np
    inv_scale = np.float32(1.0) / np.float32((new_grid + 0.1) / g)
    A = np.float32(-0.75)
    R = np.zeros((new_grid, g), dtype=np.float64)
    for o in range(new_grid):
        real = inv_scale * np.float32(o + 0.5) - np.float32(0.5)
        i = int(math.floor(real))
        t = np.float32(real - i)
        c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1          # noqa: E731
        c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A    # noqa: E731
        w = [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]
        for j, idx in enumerate(np.clip(np.arange(i - 1, i + 3), 0, g - 1)):
            R[o, idx] += float(w[j])
    return torch.from_numpy(R)


class TrainEngine:
    """Owns a `ch_model` + a `ch_trainer` for batches up to `max_batch`, and the parameter arenas: the adapters', and -- with `backbone` -- the
    backbone's (every tensor of `backbone_arena_names`; the forward then reads working copies of THAT arena, not the model's frozen weights).

    adapters: list over layers of (adapt_mlp_1, adapt_mlp_2) modules whose parameters are re-pointed into the arena.
    backbone: the `vision_model` module (or None = frozen): its parameters become views of the backbone arena the same way."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], adapters: Sequence[Sequence[torch.nn.Module]], heads: int,
                 upt_heads: int = 8, act: str = "quick_gelu", max_batch: int = 64, device=None, image_size=None, options=None,
                 backbone: torch.nn.Module = None):
        """options: ch_model_set_option settings of the frozen model the trainer is created on -- "train_chains", "train_chain_min_rows",
        "train_prune_last" are read by ch_trainer_create, "pp_min_k" etc. by every launch (ConceptHashEncoder)."""
        self.lib = _lib.load()
        # the frozen model: its own workspace is never used by training, so it is sized for one image
        self.encoder = ConceptHashEncoder(state_dict, heads=heads, upt_heads=upt_heads, act=act, max_batch=1, device=device,
                                          image_size=image_size, options=options)
        self.device = self.encoder.device
        self.cfg = self.encoder.cfg
        self.max_batch = int(max_batch)
        n = int(self.lib.ch_adapter_arena_numel(self.encoder._h))
        if n <= 0:
            raise RuntimeError("the model has no adapters: nothing to train in the encoder")
        npad = (n + 3) // 4 * 4          # ch_sgd_step works on float4s; the pad elements stay zero
        self.params = torch.zeros(npad, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros(npad, dtype=torch.float32, device=self.device)
        self._views: List[tuple] = []   # (parameter, grad view)
        D, b, L = self.cfg["dim"], self.cfg["adapter_dim"], self.cfg["layers"]
        sizes = (D, D, b * D, b, D * b, D, 1)
        if len(adapters) != L or any(len(pair) != 2 for pair in adapters):
            raise ValueError("adapters must be a list over layers of (adapt_mlp_1, adapt_mlp_2)")
        off = 0
        with torch.no_grad():
            for pair in adapters:
                for mod in pair:
                    named = dict(mod.named_parameters())
                    for field, size in zip(ADAPTER_FIELDS, sizes):
                        p = named[field]
                        if p.numel() != size:
                            raise ValueError(f"adapter parameter {field} has {p.numel()} elements, expected {size}")
                        view = self.params[off:off + size].view(p.shape)
                        view.copy_(p.detach().to(self.device, torch.float32))
                        p.data = view                     # the module's parameter IS the arena from here on
                        self._views.append((p, self.grads[off:off + size].view(p.shape)))
                        off += size
        assert off == n
        self.bparams = self.bgrads = None
        self._bviews: List[tuple] = []   # backbone (parameter, grad view)
        self._pos = None                 # position table at another resolution than the parameter's: (R, lib slot, lib grad slot, master view)
        self.fused_state = None          # state of the fused arena step (fuse_arena_step): momentum / Adam moments per arena
        if backbone is not None:
            self._adopt_backbone(backbone)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            if backbone is None:
                _lib.check(self.lib.ch_trainer_create(self.encoder._h, self.max_batch, _lib.ptr(self.params), _lib.ptr(self.grads),
                                                      ctypes.byref(h)), "ch_trainer_create")
            else:
                _lib.check(self.lib.ch_trainer_create_ex(self.encoder._h, self.max_batch, _lib.ptr(self.params), _lib.ptr(self.grads),
                                                         _lib.ptr(self.bparams), _lib.ptr(self.bgrads), ctypes.byref(h)),
                           "ch_trainer_create_ex")
        self._t = h
        self._stale = False
        # makes autograd call EncoderFunction.backward (which produces the adapters' gradients) even when nothing upstream of the
        # concept tokens requires a gradient
        self.anchor = torch.zeros((), device=self.device, requires_grad=True)
        self.generation = 0          # forwards so far: the saved activations belong to the LAST one only

    def _adopt_backbone(self, backbone: torch.nn.Module):
        """The backbone's parameters -> views of one fp32 arena in the library's layout; their `.grad`s -> views of its gradient arena.  A
        position table whose size is not the running resolution's stays the PARAMETER (kept behind the library's part of the arena, so the
        fused optimizer step still covers it); the library's slot holds its interpolation, redone at every refresh."""
        import math
        layout = backbone_arena_layout(dict(self.cfg, ln_eps=1e-5, bn_eps=1e-5))
        n = layout["__numel__"][0]
        named = dict(backbone.named_parameters())
        pos = named[POS_KEY]
        own_pos = pos.numel() != layout[POS_KEY][1]
        tail = (pos.numel() + 3) // 4 * 4 if own_pos else 0
        npad = (n + 3) // 4 * 4
        self.bparams = torch.zeros(npad + tail, dtype=torch.float32, device=self.device)
        self.bgrads = torch.zeros(npad + tail, dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for name in backbone_arena_names(self.cfg["layers"]):
                off, size = layout[name]
                p = named[name]
                if name == POS_KEY and own_pos:
                    g = int(round(math.sqrt(pos.shape[0] - 1)))
                    R = pos_interp_matrix(g, self.cfg["image_size"] // self.cfg["patch"]).to(self.device)
                    D = pos.shape[1]
                    self._pos = (R, self.bparams[off:off + size].view(-1, D), self.bgrads[off:off + size].view(-1, D))
                    off, size = npad, pos.numel()
                elif p.numel() != size:
                    raise ValueError(f"backbone parameter {name} has {p.numel()} elements, expected {size}")
                view = self.bparams[off:off + size].view(p.shape)
                view.copy_(p.detach().to(self.device, torch.float32))
                p.data = view
                self._bviews.append((p, self.bgrads[off:off + size].view(p.shape)))
        if self._pos is not None:
            self._pos = self._pos + (self._bviews[-3][0],)
            assert self._bviews[-3][0] is pos
            self._interpolate_pos()

    def _interpolate_pos(self):
        R, slot, _, master = self._pos
        with torch.no_grad():
            g = R.shape[1]
            grid = master.detach()[1:].view(g, g, -1).double()
            slot[0].copy_(master.detach()[0])
            slot[1:].copy_(torch.einsum("oy,yxd,px->opd", R, grid, R).reshape(-1, slot.shape[1]).float())

    def _pos_adjoint(self):
        """gradient of the interpolated table (what the library returns) -> gradient of the parameter: the transposed resize"""
        R, _, gslot, master = self._pos
        gview = self._bviews[-3][1]
        n = R.shape[0]
        gview[0].copy_(gslot[0])
        gview[1:].copy_(torch.einsum("oy,opd,px->yxd", R, gslot[1:].view(n, n, -1).double(), R).reshape(-1, gview.shape[1]).float())
        gslot.zero_()

    @property
    def momentum_buf(self):
        """the adapters' SGD momentum buffer, kept by the fused arena step in `fused_state` (None before its first step / under Adam)"""
        st = self.fused_state
        return st["adapter"][0] if st and st.get("kind") == "sgd" and "adapter" in st else None

    def adopt_fused_state(self, state) -> bool:
        """Take over the fused arena step's state of an earlier engine or of a checkpoint ({"kind", "step", "adapter": [...], "backbone":
        [...]}): only when every per-arena entry fits this engine's arenas; otherwise nothing is taken and the step starts afresh."""
        if not state:
            return False
        arenas = {"adapter": self.params, "backbone": self.bparams}
        for k, a in arenas.items():
            if k in state and (a is None or any(t.numel() != a.numel() for t in state[k])):
                return False
        self.fused_state = {k: ([t.to(self.device, torch.float32) for t in v] if k in arenas else v) for k, v in state.items()}
        return True

    def backbone_parameters(self) -> List[torch.nn.Parameter]:
        return [p for p, _ in self._bviews]

    def gradient_arenas(self) -> List[tuple]:
        """[(name, flat fp32 gradient arena)] the last backward filled: what a data-parallel step all-reduces in place, one collective per
        arena ("adapter", and "backbone" when the backbone trains)."""
        out = [("adapter", self.grads)]
        if self.bgrads is not None:
            out.append(("backbone", self.bgrads))
        return out

    def parameter_arenas(self) -> List[tuple]:
        out = [("adapter", self.params)]
        if self.bparams is not None:
            out.append(("backbone", self.bparams))
        return out

    def close(self):
        if getattr(self, "_t", None) is not None and self._t.value:
            self.lib.ch_trainer_destroy(self._t)
            self._t = ctypes.c_void_p()
        if getattr(self, "encoder", None) is not None:
            self.encoder.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        return int(self.lib.ch_trainer_bytes(self._t)) + self.encoder.device_bytes

    def adapter_parameters(self) -> List[torch.nn.Parameter]:
        return [p for p, _ in self._views]

    def mark_stale(self):
        """The arena changed (an optimizer step): the working copies are re-derived before the next forward."""
        self._stale = True

    def sync_versions(self):
        """In-place updates of the adapter parameters (optimizer.step(), load_state_dict) bump their tensor versions: compare
        with the versions seen at the last refresh."""
        ver = sum(p._version for p, _ in self._views) + sum(p._version for p, _ in self._bviews)
        if ver != getattr(self, "_ver", None):
            self._ver = ver
            self._stale = True

    def refresh(self, stream=None):
        if self._pos is not None:
            self._interpolate_pos()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ch_trainer_refresh(self._t, _lib.stream_ptr(stream)), "ch_trainer_refresh")
        self._stale = False

    def forward(self, images: torch.Tensor, concept_tokens: torch.Tensor, want_cls: bool = False, want_attn=False):
        """want_attn: False | True (the last layer's concept-token attention rows [B, heads, Q, Np]) | "all" (every layer's,
        [L, B, heads, Q, Np]); `backward` then takes the cotangent in the same form."""
        self.encoder._check_images(images)
        B = images.shape[0]
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds the trainer's max_batch {self.max_batch}")
        c = self.cfg
        ct = concept_tokens.detach().to(self.device, torch.float32).reshape(c["ncontext"], c["dim"]).contiguous()
        if self._stale:
            self.refresh()
        images = images.contiguous()
        hf = torch.empty(B, c["ncontext"], c["dim"], dtype=torch.float32, device=self.device)
        cls = torch.empty(B, c["dim"], dtype=torch.float32, device=self.device) if want_cls else None
        npatch = (c["image_size"] // c["patch"]) ** 2
        all_layers = want_attn == "all"
        shape = ((c["layers"],) if all_layers else ()) + (B, c["heads"], c["ncontext"], npatch)
        attn = torch.empty(shape, dtype=torch.float32, device=self.device) if want_attn else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ch_train_forward(self._t, _lib.ptr(images), 0 if images.dtype == torch.float32 else 1, B,
                                                 _lib.ptr(ct), _lib.ptr(hf), _lib.ptr(cls), _lib.ptr(attn), 1 if all_layers else 0,
                                                 _lib.stream_ptr()), "ch_train_forward")
        self.generation += 1
        return (hf, cls, attn) if want_attn else (hf, cls)

    def grads_live(self) -> bool:
        """True when the adapters' `.grad`s still are the arena views of an earlier backward, i.e. no `zero_grad()` (set_to_none,
        the default) ran since: the next backward must ADD to them, as autograd does for every other parameter."""
        return any(p.grad is not None and p.grad.data_ptr() == gview.data_ptr() for p, gview in self._views + self._bviews)

    def drop_grads(self) -> None:
        """`optimizer.zero_grad(set_to_none=True)` for the adapters alone: the next backward overwrites the arena instead of accumulating
        (what a timing loop that calls `backward` repeatedly wants -- otherwise every call after the first also pays the accumulation's
        clone + add of the arena and the gradients grow without bound)."""
        for p, _ in self._views + self._bviews:
            p.grad = None

    def backward(self, d_hash_features: torch.Tensor, d_concept_attn: torch.Tensor = None) -> torch.Tensor:
        """`ch_train_backward` OVERWRITES the gradient arena.  Gradient accumulation (two backward calls without a zero_grad in
        between: micro-batches, several losses) therefore keeps the earlier arena aside and adds it back -- the adapters then
        accumulate exactly as the head's parameters do under autograd (one extra copy + add of the arena per accumulated call)."""
        c = self.cfg
        g = d_hash_features.detach().to(self.device, torch.float32).contiguous()
        ga = d_concept_attn.detach().to(self.device, torch.float32).contiguous() if d_concept_attn is not None else None
        dct = torch.empty(c["ncontext"], c["dim"], dtype=torch.float32, device=self.device)
        live = self.grads_live()
        earlier = self.grads.clone() if live else None
        earlier_b = self.bgrads.clone() if live and self.bgrads is not None else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ch_train_backward(self._t, _lib.ptr(g), _lib.ptr(ga), _lib.ptr(dct), _lib.stream_ptr()),
                       "ch_train_backward")
        if self._pos is not None:
            self._pos_adjoint()
        if earlier is not None:
            self.grads.add_(earlier)
        if earlier_b is not None:
            self.bgrads.add_(earlier_b)
        for p, gview in self._views + self._bviews:      # optimizer.zero_grad(set_to_none=True) drops the views: put them back
            p.grad = gview
        return dct


class EncoderFunction(torch.autograd.Function):
    """hash_features = encoder(images; concept_tokens, adapters): forward / backward by the HIP library.  The adapters'
    gradients do not travel through autograd -- backward writes them into the parameters' `.grad` views (TrainEngine)."""

    @staticmethod
    def forward(ctx, concept_tokens, images, engine: TrainEngine, anchor, want_attn=False):
        """-> hash_features [B, Q, D], or (hash_features, concept_attention) with want_attn: the attention rows of the concept tokens
        over the patch tokens -- the last layer's [B, heads, Q, Np] (True) or every layer's [L, B, heads, Q, Np] ("all") --
        differentiable as well."""
        out = engine.forward(images, concept_tokens, want_attn=want_attn)     # want_attn: False | True (last layer) | "all"
        ctx.engine = engine
        ctx.generation = engine.generation
        ctx.ct_shape = concept_tokens.shape
        ctx.want_attn = want_attn
        return (out[0], out[2]) if want_attn else out[0]

    @staticmethod
    def backward(ctx, d_hf, d_attn=None):
        if ctx.generation != ctx.engine.generation:
            raise RuntimeError("EncoderFunction.backward: another training forward ran on this engine since this graph was built; the "
                               "library keeps the saved activations of the last forward only (one forward -> one backward)")
        dct = ctx.engine.backward(d_hf, d_attn if ctx.want_attn else None)
        return dct.view(ctx.ct_shape), None, None, None, None


def torch_side_parameters(model) -> List[tuple]:
    """[(name, parameter)] of the trainable parameters that are NOT views of the training engine's arenas: the concept-token generator, the
    hash head, `hash_bn`'s affine, the centre / text projection, the concept classifier (and `post_layernorm` under a trainable backbone,
    which no loss term reaches).  Deduplicated by identity (the `trainable_params.*` aliases), in `named_parameters` order -- the same on
    every rank."""
    eng = getattr(model, "_train_engine", None)
    in_arena = {id(p) for p, _ in (eng._views + eng._bviews)} if eng is not None else set()
    return [(n, p) for n, p in model.named_parameters() if p.requires_grad and id(p) not in in_arena]


def all_reduce_gradients(model, group=None, keys=None):
    """The gradient exchange of one data-parallel step, after `backward()` and before `optimizer.step()`: SUM all-reduce of the adapter
    gradient arena, of the backbone gradient arena (when the backbone trains), and of ONE flat buffer with the gradients of every
    torch-side trainable tensor -- three collectives.  Each rank scaled its loss by 1 / world_size before backward, so the sums are the
    gradients of the global-batch mean.  keys: an earlier return value (the agreed set of torch-side parameters that carry gradients), to
    skip the agreement exchange.  Returns {"keys", "bytes"}."""
    import torch.distributed as dist

    from .distributed import all_reduce_param_grads
    eng = getattr(model, "_train_engine", None)
    if eng is None:
        raise RuntimeError("all_reduce_gradients: the model has no training engine (no training forward has run)")
    nbytes = 0
    for _, arena in eng.gradient_arenas():
        dist.all_reduce(arena, op=dist.ReduceOp.SUM, group=group)
        nbytes += arena.numel() * arena.element_size()
    named = torch_side_parameters(model)
    keys = all_reduce_param_grads(named, group, keys)
    want = set(keys)
    nbytes += sum(p.numel() * p.element_size() for n, p in named if n in want)
    return {"keys": keys, "bytes": nbytes}


def fuse_adapter_sgd(optimizer, model):
    """torch.optim.SGD over the adapters = foreach kernels over 168 views of one arena (0.45 ms per step for B/16).  When the first
    param group is exactly the adapters of `model` and its training engine exists, `optimizer.step()` updates that group with ONE
    launch over the arena (`ch_sgd_step`, same arithmetic: weight decay, momentum buffer, dampening, nesterov) and lets torch step
    the remaining groups.  Anything else (another optimizer class, maximize, a closure, the engine not built yet, a missing gradient)
    falls through to the unmodified step.  Call BEFORE the lr scheduler is created (schedulers wrap `optimizer.step`)."""
    if type(optimizer) is not torch.optim.SGD:
        return optimizer
    return fuse_arena_step(optimizer, model)


def fuse_arena_step(optimizer, model):
    """`fuse_adapter_sgd` for torch.optim.SGD, Adam and AdamW, and for a trainable backbone: when param group 0 is the adapters of `model`
    -- or the whole backbone (adapters + every tensor of the backbone arena; what is left over, `post_layernorm`, stays with torch) --
    `optimizer.step()` updates it with ONE launch per arena (`ch_sgd_step` / `ch_adam_step`, torch's single-tensor arithmetic) and lets
    torch step the remaining groups.  The state (momentum, or Adam's two moments and step count) lives in `engine.fused_state`, is carried
    over engine rebuilds by the model and saved by `BaseTrainer.save_training_state`.  Anything else -- another optimizer class, amsgrad,
    maximize, capturable / tensor lr, a closure, no engine yet, a missing gradient, a group that matches neither set -- falls through to the
    unmodified step.  Call BEFORE the lr scheduler is created (schedulers wrap `optimizer.step`)."""
    kind = {torch.optim.SGD: "sgd", torch.optim.Adam: "adam", torch.optim.AdamW: "adamw"}.get(type(optimizer))
    if kind is None:
        return optimizer
    torch_step = optimizer.step
    fused = {"steps": 0}

    def arenas_of(eng, params):
        """[(key, params arena, grads arena)] that group 0 covers exactly (plus leftovers without a gradient), or None"""
        ids = {id(p) for p in params}
        ad = {id(v) for v, _ in eng._views}
        if not ad <= ids or any(v.grad is None for v, _ in eng._views):
            return None, None
        out, covered = [("adapter", eng.params, eng.grads)], set(ad)
        if eng.bparams is not None:
            bb = {id(v) for v, _ in eng._bviews}
            if bb <= ids:
                if any(v.grad is None for v, _ in eng._bviews):
                    return None, None
                out.append(("backbone", eng.bparams, eng.bgrads))
                covered |= bb
        rest = [p for p in params if id(p) not in covered]
        if any(p.grad is not None for p in rest) and len(out) == 1 and len(rest) > 0:
            return None, None          # a group that mixes the adapters with other live parameters: torch steps all of it
        return out, rest

    def step(self, closure=None):      # installed as a bound method: lr schedulers wrap `optimizer.step.__func__`
        eng = getattr(model, "_train_engine", None)
        g0 = optimizer.param_groups[0]
        params = g0["params"]
        ok = (closure is None and eng is not None and not g0.get("maximize", False) and not g0.get("amsgrad", False)
              and not g0.get("capturable", False) and not torch.is_tensor(g0["lr"]))
        arenas, rest = arenas_of(eng, params) if ok else (None, None)
        if arenas is None:
            return torch_step(closure)
        st = eng.fused_state
        if st is None or st.get("kind") != kind:
            restored = getattr(optimizer, "restored_fused_state", None)      # a checkpoint's (BaseTrainer.load_training_state)
            optimizer.restored_fused_state = None
            if not (restored and restored.get("kind") == kind and eng.adopt_fused_state(restored)):
                eng.fused_state = {"kind": kind, "step": 0}
            st = eng.fused_state
        st["step"] += 1
        with torch.cuda.device(eng.device):
            for key, pa, ga in arenas:
                if kind == "sgd":
                    first = key not in st
                    if first and g0["momentum"] != 0:
                        old = getattr(optimizer, "restored_adapter_momentum", None) if key == "adapter" else None   # checkpoints of earlier versions
                        if old is not None and old.numel() == pa.numel():
                            st[key], first = [old.to(eng.device, torch.float32).clone()], False
                            optimizer.restored_adapter_momentum = None
                        else:
                            st[key] = [torch.zeros_like(pa)]
                    buf = st[key][0] if key in st else None
                    _lib.check(eng.lib.ch_sgd_step(_lib.ptr(pa), _lib.ptr(ga), _lib.ptr(buf), pa.numel(), float(g0["lr"]),
                                                   float(g0["momentum"]), float(g0["weight_decay"]), float(g0["dampening"]),
                                                   int(bool(g0["nesterov"])), int(first), _lib.stream_ptr()), "ch_sgd_step")
                else:
                    if key not in st:
                        st[key] = [torch.zeros_like(pa), torch.zeros_like(pa)]
                    m, v = st[key]
                    _lib.check(eng.lib.ch_adam_step(_lib.ptr(pa), _lib.ptr(ga), _lib.ptr(m), _lib.ptr(v), pa.numel(), float(g0["lr"]),
                                                    float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]),
                                                    float(g0["weight_decay"]), int(kind == "adamw"), int(st["step"]), _lib.stream_ptr()),
                               "ch_adam_step")
        eng.mark_stale()                                   # the library's working copies are re-derived before the next forward
        torch.autograd.graph.increment_version(params[0])  # ... and the model's evaluation engine sees changed parameters
        fused["steps"] += 1
        g0["params"] = rest
        try:
            return torch_step()
        finally:
            g0["params"] = params

    import types
    optimizer.step = types.MethodType(step, optimizer)
    optimizer.fused_adapter_steps = fused
    return optimizer


def adapters_from_state_dict(state_dict, layers: int, dim: int, bottleneck: int) -> list:
    """Stand-alone adapter modules (parameter holders) initialised from a reference-layout state_dict: what TrainEngine needs when
    there is no model object around it (benchmarks)."""
    from models.layers.adapter import Adapter
    out = []
    for l in range(layers):
        pair = []
        for a in (1, 2):
            prefix = VM + f"encoder.layers.{l}.adapt_mlp_{a}."
            m = Adapter(dim, bottleneck)
            m.load_state_dict({k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)})
            pair.append(m)
        out.append(tuple(pair))
    return out


def backbone_from_state_dict(state_dict) -> torch.nn.Module:
    """A stand-alone `vision_model` parameter holder (module tree named as the state_dict keys below `vision_model.`, adapters left out):
    what TrainEngine(backbone=...) needs when there is no model object around it (benchmarks, engine-level tests)."""
    root = torch.nn.Module()
    for k, v in state_dict.items():
        if not k.startswith(VM) or ".adapt_mlp_" in k or not torch.is_tensor(v) or not v.is_floating_point():
            continue
        mod, parts = root, k[len(VM):].split(".")
        for name in parts[:-1]:
            if not hasattr(mod, name):
                mod.add_module(name, torch.nn.Module())
            mod = getattr(mod, name)
        mod.register_parameter(parts[-1], torch.nn.Parameter(v.detach().clone().float()))
    return root


def encoder_step_flops(cfg: dict) -> tuple:
    """(forward, backward) algorithmic FLOPs per image of the encoder's training step: the backward's input-gradient products
    equal the forward's linears, the adapters add their weight-gradient products, attention backward is 2.5x its forward."""
    D, L, M, b = cfg["dim"], cfg["layers"], cfg["ffn"], cfg["adapter_dim"]
    N = 1 + (cfg["image_size"] // cfg["patch"]) ** 2 + cfg["ncontext"]
    lin = 2.0 * N * (4 * D * D + 2 * D * M + 4 * D * b)
    attn = 4.0 * N * N * D
    return L * (lin + attn), L * (lin + 2.5 * attn + 2.0 * N * 4 * D * b)


def adapter_modules(vision_model) -> list:
    return [(layer.adapt_mlp_1, layer.adapt_mlp_2) for layer in vision_model.encoder.layers]


def full_step_setup(cfg: dict, state_dict, max_batch: int, train_backbone: bool = False):
    """(model, criterion, optimizer) of the whole training step through the drop-in surface -- the reference's train_one_batch
    (trainers/coop.py:107-131): `LGHWithFixedPrompt` in train mode, `LGHLoss` (shipped terms), torch.optim.SGD with the arena group fused.
    cfg: a concepthash_amd.synthetic.CONFIGS entry."""
    from concepthash_amd import config as cfglib
    from models.arch.coop import LGHWithFixedPrompt
    from models.backbone.clip import CLIP
    from models.loss.coop import LGHLoss
    dims = dict(hidden_size=cfg["D"], num_hidden_layers=cfg["L"], num_attention_heads=cfg["heads"], intermediate_size=cfg["M"],
                patch_size=cfg["patch"], image_size=cfg["image"], projection_dim=cfg["P"], hidden_act="quick_gelu")
    upt = cfglib.DictConfig(multi=True, num_heads=8, dropout=0.1, ensemble_method="concat", single_hash_fc=True, hash_pe=True)
    C, cd = state_dict["center"].shape
    nbit = state_dict["hash_fc.weight"].shape[0] * 4
    tp = torch.nn.Sequential(torch.nn.Linear(cd, cd), torch.nn.ReLU(), torch.nn.Linear(cd, nbit))
    model = LGHWithFixedPrompt(CLIP(dims, allow_random_init=True), nbit, C, 4, add_bn=True, upt_config=upt, fixed_center=torch.zeros(C, cd),
                               text_projection=tp, has_adapter=True, adapter_bottleneck_dim=cfg["b"], concept_reg=True)
    model.load_state_dict(state_dict)
    model = model.cuda().train()
    model.train_max_batch = max_batch
    crit = LGHLoss(margin=0.2, scale=8, loss_scales=dict(bin_logits=1, cont_logits=1, concept_logits=1), ncontext=4)
    first = model.get_backbone() if train_backbone else model.get_adapter()
    groups = [{"params": list(first.parameters())}, {"params": list(model.get_training_modules().parameters())}]
    model.requires_grad_(False)
    for g in groups:
        for p in g["params"]:
            p.requires_grad_(True)
    opt = fuse_adapter_sgd(torch.optim.SGD(groups, lr=1e-3, momentum=0.9, weight_decay=5e-4), model)
    return model, crit, opt, C


def benchmark_full_step(cfg: dict, state_dict, batches, steps: int = 10, warmup: int = 3) -> dict:
    """Wall clock of the whole training step through the drop-in surface (`full_step_setup`): forward, `LGHLoss`, `loss.backward()`,
    `torch.optim.SGD.step()` with the adapters' group fused (fuse_adapter_sgd), synchronised once per measurement."""
    import time

    from concepthash_amd import synthetic
    model, crit, opt, C = full_step_setup(cfg, state_dict, max(batches))
    out = {}
    for B in batches:
        x = synthetic.synthetic_images(B, cfg["image"]).to("cuda", torch.bfloat16)
        y = torch.randint(0, C, (B,), device="cuda")
        for it in range(warmup + steps):
            if it == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            opt.zero_grad()
            crit(model(x)[1], y).backward()
            opt.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        out[B] = {"full_step_ms": round(ms, 3), "images_per_s": round(B / ms * 1e3, 1),
                  "what": "model.train() forward + LGHLoss + backward + SGD step (adapter group fused), wall clock"}
    model._drop_train_engine()
    return out


def benchmark_ddp_step(cfg: dict, state_dict, global_batch: int, steps: int = 10, warmup: int = 3, train_backbone: bool = False) -> dict:
    """This rank's view of the data-parallel step (an initialised process group is required): global_batch / world_size images per rank,
    loss scaled by 1 / world_size, `all_reduce_gradients`, fused SGD step.  Wall clock of the whole step, and -- measured apart, on the
    gradients of the last backward -- of the gradient all-reduce alone."""
    import time

    import torch.distributed as dist

    from concepthash_amd import synthetic
    world, rank = dist.get_world_size(), dist.get_rank()
    if global_batch % world:
        raise ValueError(f"batch {global_batch} is not divisible by world_size {world}")
    B = global_batch // world
    model, crit, opt, C = full_step_setup(cfg, state_dict, B, train_backbone)
    x = synthetic.synthetic_images(global_batch, cfg["image"])[rank * B:(rank + 1) * B].to("cuda", torch.bfloat16)
    y = torch.randint(0, C, (global_batch,), generator=torch.Generator().manual_seed(0))[rank * B:(rank + 1) * B].cuda()
    keys, nbytes = None, 0
    for it in range(warmup + steps):
        if it == warmup:
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
        opt.zero_grad()
        (crit(model(x)[1], y) / world).backward()
        red = all_reduce_gradients(model, keys=keys)
        keys, nbytes = red["keys"], red["bytes"]
        opt.step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / steps * 1e3
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        all_reduce_gradients(model, keys=keys)
    torch.cuda.synchronize()
    ar_ms = (time.perf_counter() - t0) / steps * 1e3
    model._drop_train_engine()
    return {"global_batch": global_batch, "images_per_rank": B, "step_ms": round(step_ms, 3), "all_reduce_ms": round(ar_ms, 3),
            "bytes_reduced_per_step": int(nbytes), "images_per_s": round(global_batch / step_ms * 1e3, 1), "train_backbone": bool(train_backbone)}
