#!/usr/bin/env python3
"""Training-step benchmark of the ConceptHash adapters on one MI355X: encoder forward with saved
activations + backward in the HIP library, timed with HIP events around `ch_train_forward` / `ch_train_backward`; with --full also the
whole step through the drop-in surface (model.train() forward, LGHLoss, backward, SGD step).

    python tools/train_bench.py [--config vit_b16] [--batches 32,64,128,256] [--steps 10]
    python tools/train_bench.py --gpus N [--global-batch 256] [--train-backbone]      the data-parallel step on N ranks (one JSON line)
Prints one JSON line per batch size.  --gpus N starts N fresh rank processes BEFORE any GPU call of its own, as bench.py --gpus does
(at most 16); with fewer visible GPUs than ranks the ranks share GPUs and the collectives run over gloo -- a rehearsal of the layout, which
the line says (`collective_backend`, `rehearsal`), never a scaling figure.  FLOPs: forward 2 * params-touched * tokens; the backward's dgrad products equal the
forward's, the adapters' weight-gradient products add 4 N D b per layer per adapter pair, attention backward 2.5x its forward.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from concepthash_amd import synthetic
from concepthash_amd.training import TrainEngine, adapters_from_state_dict, encoder_step_flops

MAX_RANKS = 16


def ddp_launch(a) -> int:
    """start the ranks: fresh processes, before this one touches the GPU (device_count() does not initialise it)"""
    import socket
    import subprocess
    if not 1 <= a.gpus <= MAX_RANKS:
        raise SystemExit(f"--gpus {a.gpus}: between 1 and {MAX_RANKS} ranks")
    ndev = torch.cuda.device_count()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if ndev < a.gpus and "CH_DIST_BACKEND" not in env:
        print(f"[train_bench] {a.gpus} ranks requested but {ndev} GPU(s) visible: REHEARSAL -- ranks share GPUs, collectives over gloo",
              file=sys.stderr)
        env["CH_DIST_BACKEND"] = "gloo"
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=None if r == 0 else subprocess.DEVNULL) for r in range(a.gpus)]
    bad = [(r, rc) for r, rc in enumerate(p.wait() for p in procs) if rc != 0]
    if bad:
        print(f"[train_bench] ranks failed: {bad}", file=sys.stderr)
    return 1 if bad else 0


def ddp_rank(a):
    """one rank of `--gpus N`: the whole data-parallel step (concepthash_amd.training.benchmark_ddp_step); rank 0 prints the line"""
    import torch.distributed as dist

    from concepthash_amd.training import benchmark_ddp_step
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    ndev = torch.cuda.device_count()
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, ndev)
    torch.cuda.set_device(local)
    backend = os.environ.get("CH_DIST_BACKEND", "nccl")     # nccl = RCCL over xGMI; gloo only for rehearsals on fewer GPUs than ranks
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    try:
        cfg = synthetic.CONFIGS[a.config]
        sd = synthetic.synthetic_state_dict(cfg, nbit=64, nclass=200)
        res = benchmark_ddp_step(cfg, sd, a.global_batch, a.steps, a.warmup, a.train_backbone)
        t = torch.tensor([res["step_ms"], res["all_reduce_ms"]], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)             # the slowest rank's times
        if rank == 0:
            res.update(step_ms=round(float(t[0]), 3), all_reduce_ms=round(float(t[1]), 3),
                       images_per_s=round(a.global_batch / float(t[0]) * 1e3, 1))
            print(json.dumps(dict(config=a.config, n_ranks=world, n_gpus=min(world, ndev), collective_backend=dist.get_backend(),
                                  rehearsal=bool(ndev < world), **res)), flush=True)
    finally:
        dist.destroy_process_group()


def _measure(eng, x, ctx, dhf, warmup, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for it in range(warmup + steps):
        eng.drop_grads()
        ev[0].record()
        eng.forward(x, ctx)
        ev[1].record()
        eng.backward(dhf)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            tf += ev[0].elapsed_time(ev[1])
            tb += ev[1].elapsed_time(ev[2])
    return tf / steps, tb / steps


def ab(a):
    cfg = synthetic.CONFIGS[a.config]
    sd = synthetic.synthetic_state_dict(cfg, nbit=64, nclass=200)
    adapters = adapters_from_state_dict(sd, cfg["L"], cfg["D"], cfg["b"])
    batches = [int(x) for x in a.batches.split(",")]
    dev = torch.device("cuda", torch.cuda.current_device())
    variants = []
    for spec in a.ab.split(";"):
        name, _, opts = spec.partition(":")
        options = {k: int(v) for k, v in (kv.split("=") for kv in opts.split(",") if kv)}
        variants.append((name, options, TrainEngine(sd, adapters, heads=cfg["heads"], max_batch=max(batches), device=dev, options=options)))
    Q, D = 4, cfg["D"]
    ctx = torch.randn(Q, D, device="cuda") * 0.02
    grads = {}
    for B in batches:
        x = synthetic.synthetic_images(B, cfg["image"]).to("cuda", torch.bfloat16)
        dhf = torch.randn(B, Q, D, device="cuda") * 0.01
        for cycle in range(a.cycles):
            for name, options, eng in variants:
                tf, tb = _measure(eng, x, ctx, dhf, a.warmup, a.steps)
                g = eng.grads.float().clone()
                rec = {"variant": name, "options": options, "batch": B, "cycle": cycle, "forward_ms": round(tf, 3), "backward_ms": round(tb, 3),
                       "step_ms": round(tf + tb, 3)}
                if g is not None:
                    base = grads.setdefault(B, g)
                    rec["grad_rel_l2_vs_first_variant"] = float((g - base).norm() / base.norm().clamp_min(1e-30))
                print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vit_b16")
    ap.add_argument("--batches", default="32,64,128,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also time the whole step through the drop-in surface: LGHWithFixedPrompt in "
                    "train mode, LGHLoss, loss.backward(), torch.optim.SGD.step() (wall clock between synchronisations)")
    ap.add_argument("--ab", default="", help="A/B of model options in one process, interleaved: 'name:key=v,key=v;name2:key=v' "
                    "(ch_model_set_option keys; an empty option list = the defaults); one engine per variant, --cycles rounds over them")
    ap.add_argument("--cycles", type=int, default=1)
    ap.add_argument("--image-size", type=int, default=0, help="square input size other than the config's pretrain resolution (position table "
                    "interpolated; e.g. 448 = 789 tokens of ViT-B/16, which run the streaming attention kernels)")
    ap.add_argument("--train-backbone", action="store_true", help="trainable backbone (backbone_lr_scale != 0): the engine owns the second arena "
                    "pair, backward also fills the backbone's gradients; also prints the working-copy refresh and the optimizer step (fused "
                    "ch_adam_step over the arenas against torch.optim.Adam over their views)")
    ap.add_argument("--gpus", type=int, default=0, help="N >= 1: the data-parallel training step on N ranks (started here as fresh processes, or "
                    "by a launcher that sets WORLD_SIZE / RANK): step time, the gradient all-reduce on its own, bytes reduced per step")
    ap.add_argument("--global-batch", type=int, default=256, help="with --gpus: the global batch, split evenly over the ranks")
    ap.add_argument("--encode", action="store_true", help="also time ch_encode (evaluation) at the same batches and input size")
    a = ap.parse_args()
    if a.gpus:
        if "WORLD_SIZE" not in os.environ:
            sys.exit(ddp_launch(a))
        return ddp_rank(a)
    if a.ab:
        return ab(a)
    cfg = synthetic.CONFIGS[a.config]
    sd = synthetic.synthetic_state_dict(cfg, nbit=64, nclass=200)
    adapters = adapters_from_state_dict(sd, cfg["L"], cfg["D"], cfg["b"])
    batches = [int(x) for x in a.batches.split(",")]
    size = a.image_size or cfg["image"]
    backbone = None
    if a.train_backbone:
        from concepthash_amd.training import backbone_from_state_dict
        backbone = backbone_from_state_dict(sd)
    eng = TrainEngine(sd, adapters, heads=cfg["heads"], max_batch=max(batches), device=torch.device("cuda", torch.cuda.current_device()),
                      image_size=size, backbone=backbone)
    fwd_f, bwd_f = encoder_step_flops(eng.cfg)
    if a.train_backbone:   # the weight-gradient products of the four backbone GEMMs equal the forward's linears
        D_, M_, N_ = eng.cfg["dim"], eng.cfg["ffn"], eng.encoder.ntok
        bwd_f += eng.cfg["layers"] * 2.0 * N_ * (4 * D_ * D_ + 2 * D_ * M_)
    Q, D = 4, cfg["D"]
    ctx = torch.randn(Q, D, device="cuda") * 0.02
    for B in batches:
        x = synthetic.synthetic_images(B, size).to("cuda", torch.bfloat16)
        dhf = torch.randn(B, Q, D, device="cuda") * 0.01
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        tf = tb = 0.0
        for it in range(a.warmup + a.steps):
            eng.drop_grads()      # backward overwrites the arena: no accumulation clone + add inside the timed call
            ev[0].record()
            eng.forward(x, ctx)
            ev[1].record()
            eng.backward(dhf)
            ev[2].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                tf += ev[0].elapsed_time(ev[1])
                tb += ev[1].elapsed_time(ev[2])
        tf /= a.steps
        tb /= a.steps
        print(json.dumps({"config": a.config, "image_size": size, "tokens": eng.encoder.ntok, "batch": B, "forward_ms": round(tf, 3), "backward_ms": round(tb, 3),
                          "step_ms": round(tf + tb, 3), "images_per_s": round(B / (tf + tb) * 1e3, 1),
                          "forward_tflops": round(fwd_f * B / tf / 1e9, 1), "backward_tflops": round(bwd_f * B / tb / 1e9, 1),
                          "trainer_gib": round(eng.device_bytes / 2 ** 30, 2), "trainer_bytes": int(eng.lib.ch_trainer_bytes(eng._t)),
                          "train_backbone": bool(a.train_backbone)}))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.refresh()
    e0.record()
    for _ in range(a.steps):
        eng.refresh()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"config": a.config, "train_backbone": bool(a.train_backbone), "refresh_ms": round(e0.elapsed_time(e1) / a.steps, 3)}))
    if a.train_backbone:
        optimizer_step(a, eng)

    if a.encode:
        eng.close()
        from concepthash_amd.encoder import ConceptHashEncoder
        enc = ConceptHashEncoder(sd, heads=cfg["heads"], max_batch=max(batches), image_size=size)
        for B in batches:
            x = synthetic.synthetic_images(B, size).to("cuda", torch.bfloat16)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for it in range(a.warmup + a.steps):
                if it == a.warmup:
                    e0.record()
                enc.encode(x, want=("codes", "packed"))
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            print(json.dumps({"config": a.config, "image_size": size, "tokens": enc.ntok, "batch": B, "encode_ms": round(ms, 3),
                              "encode_images_per_s": round(B / ms * 1e3, 1)}))
        enc.close()
    if a.full:
        eng.close()
        full_step(a, cfg, sd, batches)


def optimizer_step(a, eng):
    """Adam over the two arenas: one ch_adam_step launch each, against torch.optim.Adam over the views (the gradients of the last backward)."""
    import time

    from concepthash_amd import _lib
    params = eng.adapter_parameters() + eng.backbone_parameters()
    opt = torch.optim.Adam(params, lr=1e-5, weight_decay=5e-4)
    res = {}
    for name in ("torch", "fused"):
        state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in (eng.params, eng.bparams)]
        for it in range(a.warmup + a.steps):
            if it == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            if name == "torch":
                opt.step()
            else:
                for (m, v), pa, ga in zip(state, (eng.params, eng.bparams), (eng.grads, eng.bgrads)):
                    _lib.check(eng.lib.ch_adam_step(_lib.ptr(pa), _lib.ptr(ga), _lib.ptr(m), _lib.ptr(v), pa.numel(), 1e-5, 0.9, 0.999, 1e-8, 5e-4,
                                                    0, it + 1, _lib.stream_ptr()), "ch_adam_step")
        torch.cuda.synchronize()
        res[name + "_adam_step_ms"] = round((time.perf_counter() - t0) / a.steps * 1e3, 3)
    print(json.dumps(dict(config=a.config, parameters=int(eng.params.numel() + eng.bparams.numel()), **res)))


def full_step(a, cfg, sd, batches):
    from concepthash_amd.training import benchmark_full_step
    for B, r in benchmark_full_step(cfg, sd, batches, a.steps, a.warmup).items():
        print(json.dumps(dict(config=a.config, batch=B, **r)))


if __name__ == "__main__":
    main()
