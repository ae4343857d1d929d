"""CPU, gloo: the host side of data-parallel training ("Training") -- the global batch sampler, the synchronised
batch normalisation and the flat-buffer gradient all-reduce of concepthash_amd/distributed.py.  Ranks are fresh child processes
(`mp.spawn`, 2 ranks, gloo); every collective of a child has a time limit (the group's `timeout`), and a child that fails ends the test
at once."""
import datetime
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = datetime.timedelta(seconds=60)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=LIMIT)


# ---- 1. sampler ---------------------------------------------------------------------------------------------------------------
def test_global_batch_sampler_partitions_every_global_batch():
    """37 items, global batch 8, 3 epochs, world_size 1 / 2 / 4: the ranks' step-i index lists concatenated in rank order are the
    single-process step-i batch; every rank has the same number of steps; 5 items are dropped per epoch; the single-process batches are the
    (seed, epoch) permutation cut as a `BatchSampler(drop_last=True)` cuts it."""
    import engine
    from torch.utils.data import BatchSampler
    n, B, seed = 37, 8, 42
    seen_perms = []
    for epoch in range(3):
        single = engine.GlobalBatchSampler(n, B, seed, 0, 1)
        single.set_epoch(epoch)
        ref = list(single)
        assert len(ref) == len(single) == n // B == 4 and all(len(b) == B for b in ref)
        flat = [i for b in ref for i in b]
        assert len(set(flat)) == 32 and set(flat) <= set(range(n))                     # the last 5 items of the permutation are dropped
        g = torch.Generator().manual_seed(engine.epoch_seed(seed, epoch))
        perm = torch.randperm(n, generator=g).tolist()
        assert ref == list(BatchSampler(perm, B, drop_last=True))                      # cut as the single-process loader cuts
        assert sorted(set(range(n)) - set(flat)) == sorted(perm[32:])
        seen_perms.append(flat)
        for world in (1, 2, 4):
            ranks = []
            for r in range(world):
                s = engine.GlobalBatchSampler(n, B, seed, r, world)
                s.set_epoch(epoch)
                ranks.append(list(s))
                assert len(ranks[-1]) == len(s) == 4 and all(len(b) == B // world for b in ranks[-1])
            for i in range(4):
                assert sum((ranks[r][i] for r in range(world)), []) == ref[i], (epoch, world, i)
    assert seen_perms[0] != seen_perms[1] != seen_perms[2]                             # another permutation every epoch
    again = engine.GlobalBatchSampler(n, B, seed, 0, 1)
    again.set_epoch(1)
    assert [i for b in again for i in b] == seen_perms[1]                              # ... and a function of (seed, epoch) alone
    other = engine.GlobalBatchSampler(n, B, seed + 1, 0, 1)
    assert [i for b in other for i in b] != seen_perms[0]
    with pytest.raises(ValueError) as e:
        engine.GlobalBatchSampler(n, 6, seed, 0, 4)
    assert "6" in str(e.value) and "4" in str(e.value)


def test_trainer_builds_the_sharded_train_loader_only_when_asked(tmp_path):
    """One process: the default train loader stays torch's shuffling DataLoader (the single-process draw stream other tests pin);
    `global_batch_sampler: true` selects the (seed, epoch) batches -- what N ranks would split between them."""
    sys.path.insert(0, ROOT)
    import engine
    from concepthash_amd.config import DictConfig
    from trainers.coop import COOPTrainer
    from utils.datasets import SyntheticHashingDataset
    for flag in (False, True):
        cfg = DictConfig(device="cpu", batch_size=8, seed=7, model=DictConfig(), dataset=DictConfig(multiclass=False),
                         global_batch_sampler=flag)
        tr = COOPTrainer(cfg)
        tr.dataset = {"train": SyntheticHashingDataset(5, size=37, image_size=4, seed=1), "test": [], "db": []}
        tr.load_dataloader()
        sampler = tr.dataloader["train"].batch_sampler
        assert isinstance(sampler, engine.GlobalBatchSampler) == flag
        if flag:
            sampler.set_epoch(2)
            got = [idx.tolist() for _, _, idx in tr.dataloader["train"]]
            ref = engine.GlobalBatchSampler(37, 8, 7, 0, 1)
            ref.set_epoch(2)
            assert got == list(ref)


def test_per_image_draws_depend_on_seed_epoch_and_index_only(tmp_path):
    """`HashingDataset.set_draw_seed`: the crop box and flip of image i are the same whatever was drawn before and in whatever order the
    images are visited (a rank that loads rows 8..15 draws for them what one process draws for rows 0..15); without it the process
    generator's stream is untouched."""
    sys.path.insert(0, ROOT)
    from utils import transforms as T
    from utils.datasets import HashingDataset
    (tmp_path / "train.txt").write_text("".join(f"img{i}.jpg {i % 3}\n" for i in range(12)))
    ds = HashingDataset(str(tmp_path), "train.txt", transform=[T.RandomResizedCrop(224, interpolation=3), T.RandomHorizontalFlip()],
                        gpu_preprocess=True)

    def draws(order):
        out = {}
        for i in order:
            with ds._image_rng(i):
                out[i] = ds._draw(300, 400)
        return out

    ds.set_draw_seed(42, 3)
    torch.manual_seed(0)
    a = draws(range(12))
    torch.manual_seed(123)
    torch.rand(5)
    b = draws(reversed(range(6, 12)))
    assert all(a[i] == b[i] for i in b) and len({str(v) for v in a.values()}) > 6
    ds.set_draw_seed(42, 4)
    assert draws(range(12)) != a                                    # another epoch, other draws
    ds.set_draw_seed(42, 3)
    torch.manual_seed(5)
    before = torch.default_generator.get_state()
    draws(range(12))
    assert torch.equal(before, torch.default_generator.get_state())  # the process generator is left as it was
    ds.set_draw_seed(None, 0)                                       # single process: the stream of the process generator, as before
    torch.manual_seed(5)
    c = draws(range(12))
    torch.manual_seed(5)
    d = {i: ds._draw(300, 400) for i in range(12)}
    assert c == d and not torch.equal(before, torch.default_generator.get_state())


# ---- 2. synchronised batch normalisation --------------------------------------------------------------------------------------
def _bn_inputs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 16, generator=g, dtype=torch.float64) * 2.0 + torch.arange(16, dtype=torch.float64) * 0.3
    dy = torch.randn(8, 16, generator=g, dtype=torch.float64)
    w = torch.randn(16, generator=g, dtype=torch.float64)
    b = torch.randn(16, generator=g, dtype=torch.float64)
    return x, dy, w, b


def _bn_module(w, b):
    bn = torch.nn.BatchNorm1d(16).double()
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
        bn.running_mean.uniform_(-1, 1, generator=torch.Generator().manual_seed(4))
        bn.running_var.uniform_(0.5, 2, generator=torch.Generator().manual_seed(5))
    return bn.train()


def _bn_worker(rank, world, port, bounds, out_dir):
    _init(rank, world, port)
    try:
        from concepthash_amd.distributed import all_reduce_param_grads, sync_batch_norm
        x, dy, w, b = _bn_inputs()
        lo, hi = bounds[rank], bounds[rank + 1]
        bn = _bn_module(w, b)
        xl = x[lo:hi].clone().requires_grad_(True)
        for step in range(2):                              # two steps: the running statistics are updated from updated ones
            y = sync_batch_norm(xl, bn)
        (y * dy[lo:hi]).sum().backward()
        all_reduce_param_grads([("weight", bn.weight), ("bias", bn.bias)])
        torch.save({"y": y.detach(), "dx": xl.grad, "dw": bn.weight.grad, "db": bn.bias.grad, "rm": bn.running_mean, "rv": bn.running_var,
                    "nbt": bn.num_batches_tracked}, os.path.join(out_dir, f"bn{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("bounds", [[0, 3, 8], [0, 0, 8], [0, 8, 8]])
def test_sync_batch_norm_matches_batchnorm1d_on_the_concatenated_batch(tmp_path, bounds):
    """Two ranks hold rows [0:3) and [3:8) of one fp64 (8, 16) input (unequal on purpose: the function weights by count), or one rank holds
    none at all: output, input gradient, all-reduced weight / bias gradients and the running statistics equal torch.nn.BatchNorm1d in
    train mode on the whole batch to 1e-12."""
    mp.spawn(_bn_worker, args=(2, _free_port(), bounds, str(tmp_path)), nprocs=2, join=True)
    x, dy, w, b = _bn_inputs()
    bn = _bn_module(w, b)
    xr = x.clone().requires_grad_(True)
    for step in range(2):
        y = bn(xr)
    (y * dy).sum().backward()
    got = [torch.load(tmp_path / f"bn{r}.pt") for r in range(2)]
    tol = 1e-12
    for r in range(2):
        lo, hi = bounds[r], bounds[r + 1]
        assert got[r]["y"].shape == (hi - lo, 16)
        assert (got[r]["y"] - y.detach()[lo:hi]).abs().max().item() <= tol if hi > lo else True
        assert (got[r]["dx"] - xr.grad[lo:hi]).abs().max().item() <= tol if hi > lo else True
        assert (got[r]["dw"] - bn.weight.grad).abs().max().item() <= tol
        assert (got[r]["db"] - bn.bias.grad).abs().max().item() <= tol
        assert (got[r]["rm"] - bn.running_mean).abs().max().item() <= tol
        assert (got[r]["rv"] - bn.running_var).abs().max().item() <= tol
        assert int(got[r]["nbt"]) == int(bn.num_batches_tracked) == 2
    assert torch.equal(got[0]["dw"], got[1]["dw"]) and torch.equal(got[0]["rv"], got[1]["rv"])


def test_sync_batch_norm_without_a_group_is_plain_batch_norm():
    """collective=False (one process, no group): the same arithmetic on the local rows, equal to BatchNorm1d to 1e-12."""
    sys.path.insert(0, ROOT)
    from concepthash_amd.distributed import sync_batch_norm
    x, dy, w, b = _bn_inputs()
    a, ref = _bn_module(w, b), _bn_module(w, b)
    xa, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yr = sync_batch_norm(xa, a), ref(xr)
    (ya * dy).sum().backward()
    (yr * dy).sum().backward()
    for p, q in ((ya, yr), (xa.grad, xr.grad), (a.weight.grad, ref.weight.grad), (a.bias.grad, ref.bias.grad),
                 (a.running_mean, ref.running_mean), (a.running_var, ref.running_var)):
        assert (p - q).abs().max().item() <= 1e-12


# ---- 3. flat-buffer gradient all-reduce -----------------------------------------------------------------------------------------
_SHAPES = [("a", (3, 5)), ("b", (7,)), ("c", ()), ("d", (2, 3, 4)), ("never", (4,)), ("half", (6,))]


def _grads_of(rank):
    g = torch.Generator().manual_seed(100 + rank)
    out = {}
    for name, shape in _SHAPES:
        dt = torch.float64 if name == "half" else torch.float32
        out[name] = torch.randn(shape, generator=g, dtype=dt)
    out["never"] = None                   # no rank has a gradient for it
    if rank == 1:
        out["b"] = None                   # one rank only
    return out


def _flat_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    try:
        from concepthash_amd.distributed import agree_grad_keys, all_reduce_param_grads
        named = []
        for (name, shape), g in zip(_SHAPES, _grads_of(rank).values()):
            p = torch.nn.Parameter(torch.zeros(shape, dtype=torch.float64 if name == "half" else torch.float32))
            p.grad = g
            named.append((name, p))
        keys = all_reduce_param_grads(named)
        assert keys == agree_grad_keys(named) == ["a", "b", "c", "d", "half"]
        first = {n: (None if p.grad is None else p.grad.clone()) for n, p in named}
        # a second step with the agreement kept: same collectives, gradients summed once more
        again = all_reduce_param_grads(named, keys=keys)
        assert again == keys
        torch.save({"first": first, "second": {n: p.grad for n, p in named}}, os.path.join(out_dir, f"flat{rank}.pt"))
        # a gradient that appears outside the agreed set is an error, not a silent skip
        named[4][1].grad = torch.ones(4)
        with pytest.raises(RuntimeError, match="never"):
            all_reduce_param_grads(named, keys=keys)
    finally:
        dist.destroy_process_group()


def test_flat_buffer_all_reduce_sums_mixed_shapes_and_missing_gradients(tmp_path):
    """Mixed shapes and two dtypes, one parameter with `grad is None` on rank 1 only, one on both: afterwards every rank's gradients are
    the elementwise sum (a missing one counted as zeros), the parameter nobody has a gradient for keeps None, and both ranks agreed on the
    same key list first."""
    mp.spawn(_flat_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    g0, g1 = _grads_of(0), _grads_of(1)
    for r in range(2):
        got = torch.load(tmp_path / f"flat{r}.pt")
        for name, _ in _SHAPES:
            if name == "never":
                assert got["first"][name] is None and got["second"][name] is None
                continue
            want = g0[name] + (g1[name] if g1[name] is not None else torch.zeros_like(g0[name]))
            assert got["first"][name].dtype == want.dtype and torch.equal(got["first"][name], want), name
            assert torch.equal(got["second"][name], want + want), name


def test_all_reduce_flat_is_one_collective(monkeypatch):
    """Many tensors, ONE all_reduce call (counted on a stand-in for the collective), values copied back into the tensors in place."""
    sys.path.insert(0, ROOT)
    from concepthash_amd import distributed as d
    calls = []

    def fake(t, op=None, group=None):
        calls.append(t.numel())
        t.mul_(3)

    monkeypatch.setattr(d.dist, "all_reduce", fake)
    ts = [torch.full(s, float(i + 1)) for i, s in enumerate([(2, 3), (5,), (), (4, 1)])]
    ptrs = [t.data_ptr() for t in ts]
    d.all_reduce_flat(ts)
    assert calls == [6 + 5 + 1 + 4]
    assert [t.data_ptr() for t in ts] == ptrs and all(torch.equal(t, torch.full(t.shape, 3.0 * (i + 1))) for i, t in enumerate(ts))


# ---- 4. the trainer's epoch loop on 2 ranks (host logic, CPU stand-in model) ------------------------------------------------------
class _TinyModel(torch.nn.Module):
    """a linear classifier on the first pixels, fp64: small enough that 2 ranks and 1 process agree to rounding"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(11)
        self.fc = torch.nn.Linear(12, 5).double()
        self.unused = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))      # never receives a gradient

    def forward(self, x):
        logits = self.fc(x.flatten(1)[:, :12].double())
        return None, {"codes": logits, "logits_cont": logits}


class _TinyCriterion(torch.nn.Module):
    losses = {}

    def forward(self, out, y):
        return torch.nn.functional.cross_entropy(out["logits_cont"], y)


def _tiny_trainer(world_flag):
    from concepthash_amd.config import DictConfig
    from concepthash_amd.distributed import all_reduce_param_grads
    from trainers.coop import COOPTrainer
    from utils.datasets import SyntheticHashingDataset

    class Trainer(COOPTrainer):
        seen = []

        def all_reduce_gradients(self):        # the stand-in model has no HIP training engine: the flat-buffer half alone
            self._grad_keys = all_reduce_param_grads(list(self.model.named_parameters()), keys=self._grad_keys)

        def train_one_batch(self, data, meters, **kw):
            self.seen.append(data[2].tolist())
            return super().train_one_batch(data, meters, **kw)

    cfg = DictConfig(device="cpu", batch_size=8, seed=5, model=DictConfig(), dataset=DictConfig(multiclass=False),
                     global_batch_sampler=world_flag)
    tr = Trainer(cfg)
    tr.dataset = {"train": SyntheticHashingDataset(5, size=37, image_size=4, seed=1), "test": [], "db": []}
    tr.load_dataloader()
    tr.model, tr.criterion = _TinyModel(), _TinyCriterion()
    tr.optimizer = torch.optim.SGD(tr.model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-3)
    tr.scheduler = torch.optim.lr_scheduler.LambdaLR(tr.optimizer, lambda e: 1.0)
    return tr


def _epoch_worker(rank, world, port, out_dir):
    _init(rank, world, port)
    try:
        tr = _tiny_trainer(False)
        assert tr.distributed and tr.collectives and tr.world_size == 2
        with torch.no_grad():
            if rank == 1:
                tr.model.fc.weight.add_(1.0)          # a start that is NOT identical: the broadcast repairs it
        tr.broadcast_model()
        meters = [tr.train_one_epoch(ep=ep) for ep in range(2)]
        assert tr.model.unused.grad is None           # no rank has a gradient for it: stays None, the optimizer skips it
        torch.save({"w": tr.model.fc.weight.detach(), "b": tr.model.fc.bias.detach(), "seen": tr.seen,
                    "loss": [m["loss"].avg for m in meters], "count": [m["loss"].count for m in meters]},
                   os.path.join(out_dir, f"ep{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_rank_epochs_equal_the_single_process_epochs(tmp_path):
    """`BaseTrainer.train_one_epoch` / `COOPTrainer.train_one_batch` on 2 gloo ranks with a stand-in fp64 model: the ranks' batches are the
    halves of the single-process batches (both epochs), a start that differs is repaired by the broadcast, the ranks end bit-identical, the
    parameters equal the single-process run's to 1e-12 (loss scaled by 1 / world_size, SUM all-reduce), the train meters are the
    sample-weighted means over all 32 images."""
    sys.path.insert(0, ROOT)
    mp.spawn(_epoch_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    tr = _tiny_trainer(True)
    assert not tr.distributed and not tr.collectives
    meters = [tr.train_one_epoch(ep=ep) for ep in range(2)]
    got = [torch.load(tmp_path / f"ep{r}.pt") for r in range(2)]
    assert len(tr.seen) == len(got[0]["seen"]) == len(got[1]["seen"]) == 8
    for i, batch in enumerate(tr.seen):
        assert got[0]["seen"][i] + got[1]["seen"][i] == batch and len(got[0]["seen"][i]) == 4
    assert torch.equal(got[0]["w"], got[1]["w"]) and torch.equal(got[0]["b"], got[1]["b"])
    assert (got[0]["w"] - tr.model.fc.weight.detach()).abs().max().item() <= 1e-12
    assert (got[0]["b"] - tr.model.fc.bias.detach()).abs().max().item() <= 1e-12
    for r in range(2):
        assert got[r]["count"] == [32, 32]
        assert all(abs(a - m["loss"].avg) <= 1e-6 for a, m in zip(got[r]["loss"], meters))     # meters accumulate fp32 values
