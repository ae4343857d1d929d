"""Gallery-sharded retrieval across the GPUs of one node (one process per GPU, ``torch.distributed``; backend
"nccl" is RCCL over xGMI on ROCm, "gloo" is used by the CPU tests of the host logic).

SURVEY.md section 8e: the gallery is row-sharded where it was encoded (rank r owns a contiguous block of global
rows), packed query codes are all-gathered (KB-MB, latency bound), each rank scans only its shard, and the small
per-shard results are exchanged:
  * top-k:  all_gather of the per-shard (idx, dist) lists, k-way merge by (distance, global index);
  * mAP:    all_gather of per-shard histogram TOTALS -> every rank computes the global "ranked before" bases of its own segments
            -> local AP terms (from the records of its one scan, or a second local scan) -> integer all_reduce of the AP
            numerators.  Bit-identical to the single-GPU result.

The per-shard compute is injected (``ops``): on GPUs it is ``concepthash_amd.retrieval`` (HIP kernels); the gloo
tests inject a CPU stand-in so that the collective choreography itself is covered without a GPU.

Data-parallel training ("Training") adds three helpers: `all_reduce_flat` (many small tensors through ONE
collective), `all_reduce_param_grads` (the torch-side parameters' gradients, key set agreed between the ranks) and
`sync_batch_norm` (batch statistics over the GLOBAL batch).
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch
import torch.distributed as dist

from . import retrieval


def shard_bounds(total_rows: int, world: int):
    """Contiguous row blocks: rank r owns [bounds[r], bounds[r+1])."""
    base, rem = divmod(total_rows, world)
    bounds = [0]
    for r in range(world):
        bounds.append(bounds[-1] + base + (1 if r < rem else 0))
    return bounds


def _all_gather_rows(t: torch.Tensor, group=None) -> torch.Tensor:
    """all_gather along dim 0 for equal-sized per-rank tensors."""
    world = dist.get_world_size(group)
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t.contiguous(), group=group)
    return out


def _all_gather_ragged(t: torch.Tensor, group=None):
    """all_gather along dim 0 when ranks hold different row counts; returns (concatenated, counts)."""
    world = dist.get_world_size(group)
    n = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n, group=group)
    counts = [int(c.item()) for c in counts]
    mx = max(counts) if counts else 0
    pad = torch.zeros((mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[: t.shape[0]] = t
    bufs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad, group=group)
    return torch.cat([b[:c] for b, c in zip(bufs, counts)], dim=0), counts


def collectives_on(group=None) -> bool:
    """True when collectives have to run: a group of more than one rank, or CH_FORCE_COLLECTIVES=1 with an initialised one-rank group
    (every collective is then an identity -- lets a single GPU exercise the RCCL backend with this module's dtypes and shapes)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or os.environ.get("CH_FORCE_COLLECTIVES") == "1"


def all_reduce_flat(tensors: Sequence[torch.Tensor], group=None) -> None:
    """SUM all-reduce of many tensors (one dtype, one device) IN PLACE through one flat buffer: one flatten, ONE collective, one foreach
    copy back -- not one collective per tensor."""
    tensors = list(tensors)
    if not tensors:
        return
    flat = torch.cat([t.reshape(-1) for t in tensors])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    torch._foreach_copy_(tensors, [v.view(t.shape) for v, t in zip(flat.split([t.numel() for t in tensors]), tensors)])


def agree_grad_keys(named_params, group=None):
    """Which of `named_params` ([(name, parameter)], the same list in the same order on every rank) carry a gradient on ANY rank: one
    small MAX all-reduce of a 0/1 mask -> the names, identical on every rank."""
    named_params = list(named_params)
    if not named_params:
        return []
    dev = named_params[0][1].device
    mask = torch.tensor([0 if p.grad is None else 1 for _, p in named_params], dtype=torch.int32, device=dev)
    dist.all_reduce(mask, op=dist.ReduceOp.MAX, group=group)
    return [name for (name, _), m in zip(named_params, mask.tolist()) if m]


def all_reduce_param_grads(named_params, group=None, keys=None):
    """SUM all-reduce of the `.grad`s of `named_params` through one flat buffer per dtype.  The ranks must enter the same collectives
    with the same sizes, so the key set is agreed first (`agree_grad_keys`; pass `keys` = an earlier agreement to skip that exchange): a
    parameter some rank has a gradient for and this rank has not (`grad is None`) contributes zeros and receives the sum; one that no rank
    has a gradient for keeps `None`, so the optimizer skips it as it does in a single process.  Returns the agreed keys."""
    named_params = list(named_params)
    if keys is None:
        keys = agree_grad_keys(named_params, group)
    want = set(keys)
    by_dtype = {}
    for name, p in named_params:
        if name not in want:
            if p.grad is not None:
                raise RuntimeError(f"all_reduce_param_grads: {name} has a gradient on this rank but is not among the agreed keys; the "
                                   f"set of parameters with gradients changed since the ranks agreed on it")
            continue
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        by_dtype.setdefault(p.grad.dtype, []).append(p.grad)
    for dt in sorted(by_dtype, key=str):
        all_reduce_flat(by_dtype[dt], group)
    return keys


def broadcast_module_state(module: torch.nn.Module, src=0, group=None) -> None:
    """Every parameter and buffer of `module` from rank `src`, one broadcast per dtype (flattened).  The values are copied into the
    parameters themselves (in place, under no_grad), so their versions move and whatever caches derived copies by version -- the training
    engine's arenas' working copies, the evaluation engine -- re-derives them."""
    by_dtype = {}
    for t in list(module.parameters()) + list(module.buffers()):
        by_dtype.setdefault(t.dtype, []).append(t)
    with torch.no_grad():
        for dt in sorted(by_dtype, key=str):
            ts = by_dtype[dt]
            flat = torch.cat([t.detach().reshape(-1) for t in ts])
            dist.broadcast(flat, src=src, group=group)
            torch._foreach_copy_(ts, [v.view(t.shape) for v, t in zip(flat.split([t.numel() for t in ts]), ts)])


class _SyncBatchNorm(torch.autograd.Function):
    """Training-mode batch normalisation of [n_local, C] rows with the statistics of ALL ranks' rows.  Forward all-reduces
    [count, sum x, sum x^2] per channel, backward [sum dy, sum dy * xhat]; both in float64 whatever the input's type (2C + 1 numbers: the
    difference sum x^2 / N - mean^2 then loses nothing an fp32 input had).  Weighted by count: ranks may hold different numbers of rows,
    zero included.  The gradients of weight and bias are this rank's LOCAL sums -- they join the all-reduce of every other parameter's."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, group, collective):
        C = x.shape[1]
        xd = x.detach().double()
        stats = torch.cat([torch.full((1,), float(x.shape[0]), dtype=torch.float64, device=x.device), xd.sum(0), (xd * xd).sum(0)])
        if collective:
            dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=group)
        n = stats[0]
        mean = stats[1:1 + C] / n
        var = (stats[1 + C:] / n - mean * mean).clamp_min(0)          # biased, what normalises
        invstd = torch.rsqrt(var + eps)
        xhat = (xd - mean) * invstd
        ctx.save_for_backward(xhat, weight, invstd, n)
        ctx.group, ctx.collective = group, collective
        ctx.mark_non_differentiable(mean, var, n)
        y = xhat * weight.detach().double() + bias.detach().double() if weight is not None else xhat
        return y.to(x.dtype), mean, var, n

    @staticmethod
    def backward(ctx, dy, _dm, _dv, _dn):
        xhat, weight, invstd, n = ctx.saved_tensors
        C = xhat.shape[1]
        dyd = dy.double()
        local = torch.cat([dyd.sum(0), (dyd * xhat).sum(0)])
        sums = local.clone()
        if ctx.collective:
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=ctx.group)
        w = weight.detach().double() if weight is not None else 1.0
        dx = w * invstd * (dyd - sums[:C] / n - xhat * (sums[C:] / n))
        dw = local[C:].to(weight.dtype) if weight is not None else None
        db = local[:C].to(weight.dtype) if weight is not None else None
        return dx.to(dy.dtype), dw, db, None, None, None


def sync_batch_norm(x: torch.Tensor, bn: torch.nn.BatchNorm1d, group=None, collective=None) -> torch.Tensor:
    """`bn(x)` in train mode with the batch statistics taken over every rank's rows (x: [n_local, C]).  Running mean / variance are
    updated from the GLOBAL statistics with the global count by torch's rule (unbiased variance N / (N - 1), `momentum`, or the
    cumulative average when momentum is None).  collective: None = `collectives_on(group)`; False runs the same arithmetic on the local
    rows alone."""
    if collective is None:
        collective = collectives_on(group)
    y, mean, var, n = _SyncBatchNorm.apply(x, bn.weight, bn.bias, float(bn.eps), group, bool(collective))
    if bn.track_running_stats and bn.running_mean is not None:
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
            m = bn.momentum if bn.momentum is not None else 1.0 / bn.num_batches_tracked.double()
            unbiased = var * (n / (n - 1).clamp_min(1))
            bn.running_mean.copy_(((1 - m) * bn.running_mean.double() + m * mean).to(bn.running_mean.dtype))
            bn.running_var.copy_(((1 - m) * bn.running_var.double() + m * unbiased).to(bn.running_var.dtype))
    return y


class RowShard:
    """This rank's block of an [N, ...] tensor whose rows are sharded over the ranks in contiguous, rank-major (= dataset) order --
    what `BaseTrainer.inference_one_epoch` returns per output in a multi-rank run: the codes STAY on the GPU that encoded them
    (SURVEY.md section 8e "shards where it was encoded, no movement"), `utils.hashing` scans them in place, and only
    `gather()` (for `save_code`) moves them.  Supports the handful of tensor operations the evaluator applies to its outputs
    (experiments/test_hashing.py:76-103): `clone`, `dim`, `size`, `shape`, column selection `x[:, cols]`, `x - row`, `mean(dim=0)`,
    and row-wise maps."""

    def __init__(self, local: torch.Tensor, counts=None, group=None):
        self.local, self.group = local, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        if counts is None:
            n = torch.tensor([local.shape[0]], dtype=torch.int64, device=local.device)
            got = [torch.zeros_like(n) for _ in range(self.world)]
            dist.all_gather(got, n, group=group)
            counts = [int(c.item()) for c in got]
        self.counts = list(counts)
        assert self.counts[self.rank] == local.shape[0]

    # ---- tensor-like surface ---------------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return torch.Size((sum(self.counts),) + tuple(self.local.shape[1:]))

    @property
    def dtype(self):
        return self.local.dtype

    @property
    def device(self):
        return self.local.device

    @property
    def offset(self):
        return sum(self.counts[: self.rank])

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    def dim(self):
        return self.local.dim()

    def __len__(self):
        return sum(self.counts)

    def map(self, fn):
        """row-wise function of the local block (must keep the row count)"""
        out = fn(self.local)
        assert out.shape[0] == self.local.shape[0]
        return RowShard(out, self.counts, self.group)

    def clone(self):
        return self.map(lambda t: t.clone())

    def __getitem__(self, idx):
        if not (isinstance(idx, tuple) and len(idx) == 2 and idx[0] == slice(None)):
            raise IndexError("RowShard supports column selection x[:, cols] only (rows live on different ranks)")
        cols = idx[1].to(self.local.device) if torch.is_tensor(idx[1]) else idx[1]
        return self.map(lambda t: t[:, cols])

    def __sub__(self, other):
        return self.map(lambda t: t - torch.as_tensor(other).to(t.device))

    def mean(self, dim=0, keepdim=False):
        """Column mean over ALL rows with the arithmetic of the single-process evaluator (torch.mean of the whole CPU tensor, the
        reference's `db_codes.mean(dim=0, keepdim=True)`): computed on rank 0 from the gathered rows and broadcast, so that
        `zero_mean_eval` gives the same bits for any rank count.  The one option that moves codes; off in the shipped configs."""
        if dim != 0:
            raise NotImplementedError("RowShard.mean: dim=0 only")
        full = self.gather(dst=0)
        box = [full.mean(dim=0, keepdim=keepdim) if self.rank == 0 else None]
        dist.broadcast_object_list(box, src=0, group=self.group)
        return box[0]

    def gather(self, dst=0):
        """The whole tensor on the host of rank `dst` (None on the other ranks); dst=None: on every rank.  No rank other than
        `dst` copies anything to its host."""
        full, _ = _all_gather_ragged(self.local.contiguous(), self.group)
        if dst is None or self.rank == dst:
            return full.cpu()
        return None


def gather_outputs(outputs: dict, dst=0):
    """{name: RowShard | anything} -> the same dict with every RowShard gathered to rank `dst` (for `save_code`)."""
    return {k: (v.gather(dst) if isinstance(v, RowShard) else v) for k, v in outputs.items()}


class ShardedRetrieval(retrieval.WholeGallery):
    """Rank-local view of a row-sharded gallery.

    gallery:  packed codes of THIS rank's rows, int64 [G_local, W]
    labels:   labels of this rank's rows (1-D class ids or 2-D indicator matrix), optional
    ops:      module/object providing hamming_topk, topk_merge, prepare_labels, labels_single, hamming_hist, hist_prefix,
              hamming_ap_multi, normalize_limits, summarize, map_seg_rows -- and, for the one-scan form, hamming_hist_rec /
              hamming_ap_rec  (default: concepthash_amd.retrieval)

    A `retrieval.WholeGallery` whose cross-rank steps are collectives: `evaluate` runs `retrieval.evaluate_gallery` on it.
    """

    def __init__(self, gallery: torch.Tensor, labels: Optional[torch.Tensor] = None, group=None, ops=None):
        if not dist.is_initialized():
            raise RuntimeError("ShardedRetrieval needs an initialised torch.distributed process group")
        super().__init__(gallery.contiguous(), labels, retrieval if ops is None else ops)
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        dev = gallery.device
        n = torch.tensor([gallery.shape[0]], dtype=torch.int64, device=dev)
        counts = [torch.zeros_like(n) for _ in range(self.world)]
        dist.all_gather(counts, n, group=group)
        self.counts = [int(c.item()) for c in counts]
        self.base = sum(self.counts[: self.rank])       # global index of this shard's first row
        self.total = self.rows = sum(self.counts)
        self.scan_rows = max(max(self.counts), 1)       # one segment size for all ranks, chosen for the largest shard
        # CH_FORCE_COLLECTIVES=1: run every collective also in a one-rank group (they are then identities) -- lets a single GPU
        # exercise the RCCL backend with this module's dtypes and shapes (tests/test_parity_r3_gpu.py)
        self.coll = self.world > 1 or os.environ.get("CH_FORCE_COLLECTIVES") == "1"

    # ---- queries -------------------------------------------------------------------------------------------------
    def gather_queries(self, q_local: torch.Tensor) -> torch.Tensor:
        """Queries encoded on different ranks -> the full query set on every rank (rank-major order)."""
        allq, _ = _all_gather_ragged(q_local, self.group)
        return allq

    # ---- top-k ---------------------------------------------------------------------------------------------------
    def topk(self, q_all: torch.Tensor, k: int):
        """q_all: the SAME [Qn, W] on every rank.  Returns the global (idx int64 [Qn,k], dist int32 [Qn,k]) on every rank."""
        idx, dst = self.ops.hamming_topk(q_all, self.gallery, k, g_index_base=self.base)
        if not self.coll:
            return idx, dst
        li = _all_gather_rows(idx.unsqueeze(0), self.group)   # [world, Qn, k]
        ld = _all_gather_rows(dst.unsqueeze(0), self.group)
        return self.ops.topk_merge(li, ld)

    # ---- mAP / P@k / R@k -----------------------------------------------------------------------------------------
    def evaluate(self, q_all: torch.Tensor, q_labels: torch.Tensor, R=-1, ks: Sequence[int] = (1, 5, 10),
                 remove_first: bool = False, seg_rows: Optional[int] = None, skip_queries_without_relevant: bool = False,
                 tie_bracket: bool = False, radii: Optional[Sequence[int]] = None, tie_expected: bool = False) -> dict:
        """Same statistics as ``retrieval.evaluate`` (R an int or a list; `skip_queries_without_relevant` as there), gallery sharded by rows: per-shard histograms are
        all-gathered, every rank builds the same global bases, ONE local AP pass accumulates every rank limit (each R and each
        k), and the integer sums are all-reduced -- bit-identical to the single-GPU result for any shard count.
        tie_bracket: as ``retrieval.evaluate``: the whole-gallery bucket counts are the sum over ranks of the per-shard totals that were
        all-gathered anyway, and every rank runs the bracket kernel on the same integers (replicated; no further collective).
        tie_expected: as ``retrieval.evaluate``, from the same summed integers after they have crossed the ranks: every rank runs the
        expectation kernel on identical counts, so any sharding gives the single-process bits.
        radii (hash lookup, ``retrieval.hash_lookup_stats``): not built for the sharded evaluator."""
        if radii is not None:
            raise NotImplementedError("ShardedRetrieval.evaluate(radii=...): hash lookup is not built for a sharded gallery (it would take "
                                      "one all-reduce of the [Qn, nb, 2] bucket counts); evaluate on one GPU with retrieval.evaluate")
        if self.labels is None:
            raise ValueError("gallery labels are required for evaluate()")
        # one-hot rows -> class ids only if EVERY shard's rows (and the queries) are single-label: the ranks must agree on the form
        single = None
        if self.coll and q_labels.dim() == 2 and self.labels.dim() == 2:
            dev = q_all.device
            flag = torch.tensor([1 if self.ops.labels_single(q_labels.to(dev), self.labels.to(dev)) else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
            single = bool(flag.item())
        return retrieval.evaluate_gallery(self, q_all, q_labels, R, ks, remove_first, seg_rows, None, None, skip_queries_without_relevant,
                                          tie_bracket, None, single, tie_expected=tie_expected)

    # ---- the steps of `retrieval.evaluate_gallery` that cross ranks ------------------------------------------------
    def first_relevant(self, q_all, q_lab, g_lab, LW):
        """relevance of the global rank-1 row of every query"""
        idx, _ = self.topk(q_all, 1)
        g_lab_all, _ = _all_gather_ragged(g_lab, self.group) if self.coll else (g_lab, None)
        return retrieval._relevance_of(idx, q_lab, g_lab_all, LW)[:, 0].to(torch.int32)

    def bases(self, hist, want_counts):
        if not self.coll:
            return super().bases(hist, want_counts)
        # "ranked before" bases of THIS shard's segments need, per (query, bucket), the rows of all lower buckets anywhere plus
        # the same bucket's rows in earlier shards and earlier local segments: only per-SHARD totals travel ([Qn, nb, 2] per
        # rank -- 17 MB at 16,384 queries x 128 bit -- instead of every segment's histogram, 16x that at the 1M-row size), and
        # the prefix runs over [all earlier shards | local segments | all later shards]
        tot = hist.sum(0, dtype=hist.dtype)
        tot_all = _all_gather_rows(tot.unsqueeze(0), self.group)                        # [world, Qn, nb, 2], rank-major
        before = tot_all[: self.rank].sum(0, dtype=hist.dtype)
        after = tot_all[self.rank + 1:].sum(0, dtype=hist.dtype)
        base_s, totals = self.ops.hist_prefix(torch.cat([before.unsqueeze(0), hist, after.unsqueeze(0)], dim=0))
        return base_s[1:1 + hist.shape[0]].contiguous(), totals, tot_all.sum(0, dtype=hist.dtype) if want_counts else None

    def reduce(self, S, nrel):
        if self.coll:
            dist.all_reduce(S, op=dist.ReduceOp.SUM, group=self.group)       # int64 wrap-around sum == uint64 sum
            dist.all_reduce(nrel, op=dist.ReduceOp.SUM, group=self.group)
