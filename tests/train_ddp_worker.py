"""Child process of tests/test_train_ddp_gpu.py: builds the `exp=hashing` experiment from the composed config exactly as main_v2.py does
(RetrievalExperiment: trainer, datasets, loaders, model, optimizer, criterion) and drives a few training steps by hand, so that the state
after EVERY step can be inspected.

    python train_ddp_worker.py <out.pt> <mode> <steps> [config overrides ...]

mode  single    one process, the global batches of the (seed, epoch) sampler (`global_batch_sampler=true`)
      reversed  the same, every batch's rows in reverse order: the same sums in another floating-point order
      ranks     one rank of a multi-rank group (launcher environment: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT, CH_DIST_BACKEND)
      solo      a ONE-rank group (backend from CH_DIST_BACKEND, default nccl = RCCL); with CH_FORCE_COLLECTIVES=1 every collective of the
                step runs, without it the same arithmetic runs with the collectives skipped (`hash_bn_sync` forced on)
"""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def checksum(t: torch.Tensor) -> torch.Tensor:
    """64-bit position-weighted checksum of a tensor's bit patterns (int64 wrap-around arithmetic), on the tensor's device"""
    bits = t.detach().contiguous().view(-1).view(torch.int32 if t.element_size() == 4 else torch.int64).to(torch.int64)
    weight = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 65521 + 1
    return (bits * weight).sum()


def buffers_of(model):
    """name -> tensor: the parameter arenas and every torch-side trainable parameter, plus the batch-norm running statistics"""
    from concepthash_amd.training import torch_side_parameters
    out = {"arena/" + n: a for n, a in model._train_engine.parameter_arenas()}
    out.update({"torch/" + n: p for n, p in torch_side_parameters(model)})
    out.update({"stat/" + n: b for n, b in model.hash_bn.named_buffers()})
    return out


def main():
    out_path, mode, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
    overrides = sys.argv[4:]
    from concepthash_amd import config as cfglib
    torch.cuda.set_device(0)
    if mode in ("ranks", "solo"):
        backend = os.environ.get("CH_DIST_BACKEND", "nccl")
        if mode == "solo":
            os.environ.update(RANK="0", WORLD_SIZE="1")
        kw = dict(device_id=torch.device("cuda", 0)) if backend == "nccl" else {}
        dist.init_process_group(backend, timeout=datetime.timedelta(seconds=120), **kw)
    if mode in ("single", "reversed", "solo"):
        overrides = overrides + ["global_batch_sampler=true"]
    config = cfglib.compose(os.path.join(ROOT, "configs"), "train.yaml", overrides, cwd=os.getcwd())
    from experiments.train_helper import RetrievalExperiment
    from utils.misc import DeviceMeters
    exp = RetrievalExperiment(config)
    tr = exp.trainer
    if mode == "solo":
        tr.model.hash_bn_sync = True
    tr.model.train()
    tr.criterion.train()
    trainable = [(n, p) for n, p in tr.model.named_parameters() if p.requires_grad]
    start = {n: p.detach().cpu().clone() for n, p in trainable} if mode == "single" else None
    calls = {"all_reduce": 0}
    if dist.is_initialized():
        real = dist.all_reduce

        def counted(t, *a, **k):
            calls["all_reduce"] += 1
            assert t.is_cuda
            return real(t, *a, **k)
        dist.all_reduce = counted
    loader = tr.dataloader["train"]
    loader.batch_sampler.set_epoch(0)
    meters = DeviceMeters(tr.device)
    indices, losses = [], []
    for i, (image, labels, index) in enumerate(loader):
        if i == steps:
            break
        if mode == "reversed":
            image, labels, index = image.flip(0), labels.flip(0), index.flip(0)
        indices.append(index.clone())
        tr.train_one_batch((image, labels, index), meters, bidx=i)
        if mode == "ranks":
            # (a) after each step the ranks hold bit-identical parameters: all_gather of one 64-bit checksum per buffer
            bufs = buffers_of(tr.model)
            mine = torch.stack([checksum(t) for t in bufs.values()])
            got = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
            dist.all_gather(got, mine)
            for r, other in enumerate(got):
                bad = [n for n, a, b in zip(bufs, mine.tolist(), other.tolist()) if a != b]
                assert not bad, f"step {i}: rank {dist.get_rank()} and rank {r} differ in {bad[:5]}"
    torch.cuda.synchronize()
    final = meters.finalize()
    state = {k: v.detach().cpu().clone() for k, v in buffers_of(tr.model).items()}
    # the size of the three steps' update itself, per group of parameters: what a fault that rescales or drops a gradient changes
    moved = None
    if start is not None:
        eng = tr.model._train_engine
        group = {id(p): "adapter" for p, _ in eng._views}
        group.update({id(p): "backbone" for p, _ in eng._bviews})
        moved = {n: (group.get(id(p), "torch_side"), p.detach().cpu().clone(), start[n]) for n, p in trainable}
    torch.save({"state": state, "indices": indices, "moved": moved, "loss": final["loss"].avg, "all_reduce_calls": calls["all_reduce"],
                "fused_steps": tr.optimizer.fused_adapter_steps["steps"]}, out_path)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    print("WORKER_OK")


if __name__ == "__main__":
    main()
