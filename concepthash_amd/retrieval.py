"""Packed-code Hamming retrieval on the GPU through the C-ABI: pack, distance, top-k, mAP / P@k / R@k, and the
gallery-sharded multi-GPU variants (one process per GPU, RCCL via ``torch.distributed``).

Replaces the reference's un-vendored ``utils.hashing`` arithmetic (call sites experiments/test_hashing.py:106-119,
153-162).  PyTorch supplies device buffers, streams and collectives; all per-pair arithmetic runs in
``csrc/hamming_topk.hip`` (top-k search), ``csrc/hamming.hip`` (distance matrix, mAP) and ``csrc/hamming_rankcount.hip`` (mAP under the weighted distance) and ``csrc/hamming_ternary.hip`` (ternary codes: two bit planes per row, [rows, 2, W]); ``csrc/dense_rank.hip`` ranks the real-valued codes themselves (cosine / Euclidean / dot).  Packed codes are ``int64`` tensors holding the uint64 bit patterns ([rows, W]).
"""
from __future__ import annotations

import ctypes
import os
import sys
from typing import Optional, Sequence, Tuple

import torch

from . import _lib

TWO32 = 4294967296.0


def _dev_guard(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("retrieval kernels need GPU tensors (MI355X); there is no CPU fallback")
    return torch.cuda.device(t.device)


def pack_sign(codes: torch.Tensor, threshold: float = 0.0, stream=None) -> torch.Tensor:
    """[rows, nbit] fp32 -> [rows, ceil(nbit/64)] int64; bit i = (codes[:, i] - threshold) > 0 (little endian)."""
    lib = _lib.load()
    if codes.dim() != 2:
        raise ValueError("codes must be 2-D")
    codes = codes.to(torch.float32).contiguous()
    rows, nbit = codes.shape
    out = torch.empty(rows, (nbit + 63) // 64, dtype=torch.int64, device=codes.device)
    with _dev_guard(codes):
        _lib.check(lib.ch_pack_sign(_lib.ptr(codes), rows, nbit, float(threshold), _lib.ptr(out), _lib.stream_ptr(stream)),
                   "ch_pack_sign")
    return out


def _check_packed(q: torch.Tensor, g: torch.Tensor):
    if q.dtype != torch.int64 or g.dtype != torch.int64 or q.dim() != 2 or g.dim() != 2:
        raise TypeError("packed codes must be 2-D int64 tensors")
    if q.shape[1] != g.shape[1]:
        raise ValueError(f"query has {q.shape[1]} words per code, gallery {g.shape[1]}")
    if q.device != g.device:
        raise ValueError("query and gallery codes must be on the same device")
    return q.contiguous(), g.contiguous()


def hamming_dist(q: torch.Tensor, g: torch.Tensor, stream=None) -> torch.Tensor:
    """Full [Qn, G] int32 distance matrix (small problems; ``get_hamm_dist`` semantics without normalisation)."""
    lib = _lib.load()
    q, g = _check_packed(q, g)
    out = torch.empty(q.shape[0], g.shape[0], dtype=torch.int32, device=q.device)
    with _dev_guard(q):
        _lib.check(lib.ch_hamming_dist(_lib.ptr(q), q.shape[0], _lib.ptr(g), g.shape[0], q.shape[1], _lib.ptr(out),
                                       _lib.stream_ptr(stream)), "ch_hamming_dist")
    return out


def _check_mask(mask: torch.Tensor, Qn: int, W: int, device, whose: str) -> Tuple[torch.Tensor, int]:
    """A query mask, int64 [W] (one for all queries) or [Qn, W] (one per query) -> (contiguous mask, its row stride: 0 or W)."""
    if mask.dtype != torch.int64 or mask.device != device or tuple(mask.shape) not in ((W,), (Qn, W)):
        raise ValueError(f"mask must be an int64 tensor [{W}] or [{Qn}, {W}] on the {whose}' device, got {mask.dtype} "
                         f"{tuple(mask.shape)} on {mask.device}")
    return mask.contiguous(), 0 if mask.dim() == 1 else W


def _topk(entry: str, q: torch.Tensor, g: torch.Tensor, k: int, g_index_base: int, stream, operands=(),
          workspace: str = "ch_hamming_topk_workspace", filt=(), behind_w=()) -> Tuple[torch.Tensor, torch.Tensor]:
    """The call of a ch_hamming_topk* / ch_ternary_topk* entry on checked codes ([rows, W] or [rows, 2, W]): allocates idx / dist / the
    workspace; `operands` are the entry's own arguments between q and Qn, `behind_w` those between W and k (the ternary nbit); `filt`
    those of a filtered entry (`_check_filter`), behind g_index_base."""
    lib = _lib.load()
    Qn, W, G = q.shape[0], q.shape[-1], g.shape[0]
    idx = torch.empty(Qn, k, dtype=torch.int64, device=q.device)
    dist = torch.empty(Qn, k, dtype=torch.int32, device=q.device)
    wsb = int(getattr(lib, workspace)(Qn, G, W, k))
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    with _dev_guard(q):
        _lib.check(getattr(lib, entry)(_lib.ptr(q), *operands, Qn, _lib.ptr(g), G, W, *behind_w, k, int(g_index_base), *_filter_args(filt),
                                       _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(ws), wsb, _lib.stream_ptr(stream)), entry)
    return idx, dist


def hamming_topk(q: torch.Tensor, g: torch.Tensor, k: int, g_index_base: int = 0, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k by ascending (distance, gallery index): (idx int64 [Qn,k], dist int32 [Qn,k]); -1 where k > G."""
    q, g = _check_packed(q, g)
    return _topk("ch_hamming_topk", q, g, k, g_index_base, stream)


def hamming_topk_masked(q: torch.Tensor, g: torch.Tensor, mask: torch.Tensor, k: int, g_index_base: int = 0,
                        stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """hamming_topk with dist = popcount((q ^ g) & mask).  mask: int64 [W] (one mask for all queries, e.g. `concept_mask`) or
    [Qn, W] (one per query, e.g. `confidence_mask`).  Bits of the last word past nbit count unless the codes or the mask clear them
    (`pack_sign` leaves them zero)."""
    q, g = _check_packed(q, g)
    mask, stride = _check_mask(mask, q.shape[0], q.shape[1], q.device, "queries")
    return _topk("ch_hamming_topk_masked", q, g, k, g_index_base, stream, (_lib.ptr(mask), stride))


WEIGHT_BITS = (4, 8)


def weight_planes(codes: torch.Tensor, bits: int = 8, mask: Optional[torch.Tensor] = None, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The query side of the weighted (asymmetric) distance: [Qn, nbit] fp32 codes -> (planes int64 [Qn, bits, W], wsum int32 [Qn]).
    w = floor(|code| L / max|code| + 0.5) per query, L = 2^bits - 1, evaluated in fp64; |code| counts as 0 where it is not finite or
    the mask clears the bit (mask: int64 [W] or [Qn, W], as `hamming_topk_masked` takes); bit b of planes[i, p, w] is bit p of the
    weight of code bit 64 w + b; wsum is the sum of a query's weights = the largest distance it can reach."""
    lib = _lib.load()
    if codes.dim() != 2:
        raise ValueError("codes must be 2-D")
    if int(bits) not in WEIGHT_BITS:
        raise ValueError(f"weight bits must be one of {WEIGHT_BITS}, got {bits}")
    codes = codes.to(torch.float32).contiguous()
    Qn, nbit = codes.shape
    W = (nbit + 63) // 64
    stride = 0
    if mask is not None:
        mask, stride = _check_mask(mask, Qn, W, codes.device, "codes")
    planes = torch.empty(Qn, int(bits), W, dtype=torch.int64, device=codes.device)
    wsum = torch.empty(Qn, dtype=torch.int32, device=codes.device)
    with _dev_guard(codes):
        _lib.check(lib.ch_weight_planes(_lib.ptr(codes), Qn, nbit, _lib.ptr(mask), stride, int(bits), _lib.ptr(planes), _lib.ptr(wsum),
                                        _lib.stream_ptr(stream)), "ch_weight_planes")
    return planes, wsum


def hamming_topk_weighted(q: torch.Tensor, planes: torch.Tensor, g: torch.Tensor, k: int, g_index_base: int = 0,
                          stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """hamming_topk with dist = sum_p 2^p popcount((q ^ g) & planes[:, p]): the weighted distance of `weight_planes(codes)` with
    q = pack_sign(codes).  Lists of gallery shards merge with `topk_merge` as the unweighted ones do."""
    q, planes, g = _check_weighted(q, planes, g)
    return _topk("ch_hamming_topk_weighted", q, g, k, g_index_base, stream, (_lib.ptr(planes), planes.shape[1]),
                 workspace="ch_hamming_topk_weighted_workspace")


# ---------------------------------------------------------------------------------------------------------------
# filtered search: the top-k among admitted rows only ("filtered search")
# ---------------------------------------------------------------------------------------------------------------
def row_bitmap(allow: torch.Tensor) -> torch.Tensor:
    """bool [G] (on any device, the CPU included: torch ops only) -> int64 [ceil(G / 64)], the allow-list of the filtered entries: bit
    r & 63 of word r >> 6 is allow[r]; the bits past G in the last word are zero."""
    if allow.dtype != torch.bool or allow.dim() != 1:
        raise TypeError(f"allow must be a bool tensor [G], got {allow.dtype} {tuple(allow.shape)}")
    G = allow.shape[0]
    words = (G + 63) // 64
    bits = torch.zeros(words * 64, dtype=torch.int64, device=allow.device)
    bits[:G] = allow
    shifts = torch.arange(64, dtype=torch.int64, device=allow.device)
    return (bits.view(words, 64) << shifts[None, :]).sum(1)           # distinct bits: the sum is their OR (bit 63 = the sign)


def bitmap_count(bitmap: torch.Tensor, G: int) -> int:
    """The set bits among the first G of a `row_bitmap` (what lies past G in the last word is not counted)."""
    shifts = torch.arange(64, dtype=torch.int64, device=bitmap.device)
    return int(((bitmap[:, None] >> shifts[None, :]) & 1).reshape(-1)[:G].sum())


def _check_filter(allow, group, want, exclude, Qn: int, G: int, device):
    """The filter of a filtered entry on checked codes -> (bitmap or None, group or None, want or None, exclude).  allow: bool [G]
    (packed here) or a packed int64 [ceil(G / 64)]; group: int32 [G]; want: int64 [Qn]; all on the codes' device."""
    if not isinstance(exclude, bool):
        raise TypeError(f"exclude must be a bool, got {exclude!r}")
    words = (G + 63) // 64
    if allow is not None:
        if not isinstance(allow, torch.Tensor) or allow.device != device or \
                (allow.dtype, tuple(allow.shape)) not in ((torch.bool, (G,)), (torch.int64, (words,))):
            raise ValueError(f"allow must be a bool tensor [{G}] or a packed int64 bitmap [{words}] (row_bitmap) on the codes' device, got "
                             f"{getattr(allow, 'dtype', type(allow))} {tuple(getattr(allow, 'shape', ()))} on {getattr(allow, 'device', None)}")
        allow = row_bitmap(allow) if allow.dtype == torch.bool else allow.contiguous()
    if group is not None:
        if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or tuple(group.shape) != (G,) or group.device != device:
            raise ValueError(f"group must be an int32 tensor [{G}] on the codes' device, got {getattr(group, 'dtype', type(group))} "
                             f"{tuple(getattr(group, 'shape', ()))} on {getattr(group, 'device', None)}")
        if want is None:
            raise ValueError("group without want: a group plane is read for the queries' wanted groups, int64 [Qn]")
        group = group.contiguous()
    if want is not None:
        if not isinstance(want, torch.Tensor) or want.dtype != torch.int64 or tuple(want.shape) != (Qn,) or want.device != device:
            raise ValueError(f"want must be an int64 tensor [{Qn}] on the codes' device (-1 = no group filter for that query), got "
                             f"{getattr(want, 'dtype', type(want))} {tuple(getattr(want, 'shape', ()))} on {getattr(want, 'device', None)}")
        want = want.contiguous()
    return allow, group, want, exclude


def _filter_args(filt):
    """allow, group, want, exclude of a C entry; () for the unfiltered ones"""
    if not filt:
        return ()
    allow, group, want, exclude = filt
    return _lib.ptr(allow), _lib.ptr(group), _lib.ptr(want), int(exclude)


def hamming_topk_filtered(q: torch.Tensor, g: torch.Tensor, k: int, allow: Optional[torch.Tensor] = None,
                          group: Optional[torch.Tensor] = None, want: Optional[torch.Tensor] = None, exclude: bool = False,
                          mask: Optional[torch.Tensor] = None, planes: Optional[torch.Tensor] = None, g_index_base: int = 0,
                          stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`hamming_topk` (neither mask nor planes), `hamming_topk_masked` (mask) or `hamming_topk_weighted` (planes) among ADMITTED rows only:
    the k smallest by ascending (distance, global index) of the rows that pass the filter, -1 behind them where fewer than k do.
    Row r of THIS gallery is admitted for query i iff
      allow is None or allow[r] -- bool [G], or the packed int64 [ceil(G / 64)] of `row_bitmap` (bits past G are ignored) -- and
      want is None or want[i] < 0 or (grp(r) == want[i]) != exclude, with grp(r) = group[r] (int32 [G], values >= 0) or, without a group
      plane, g_index_base + r: a row is its own group, so want = the query's own global index and exclude=True drops exactly that row.
    With every row admitted the result equals the unfiltered entry's bit for bit; lists of gallery shards (each with its own base,
    bitmap and slice of group) merge with `topk_merge`."""
    if planes is not None:
        if mask is not None:
            raise ValueError("mask with planes: the planes of `weight_planes(codes, bits, mask)` already carry the mask")
        q, planes, g = _check_weighted(q, planes, g)
    else:
        q, g = _check_packed(q, g)
    filt = _check_filter(allow, group, want, exclude, q.shape[0], g.shape[0], q.device)
    if planes is not None:
        return _topk("ch_hamming_topk_weighted_filtered", q, g, k, g_index_base, stream, (_lib.ptr(planes), planes.shape[1]),
                     workspace="ch_hamming_topk_weighted_filtered_workspace", filt=filt)
    stride = 0
    if mask is not None:
        mask, stride = _check_mask(mask, q.shape[0], q.shape[1], q.device, "queries")
    return _topk("ch_hamming_topk_filtered", q, g, k, g_index_base, stream, (_lib.ptr(mask), stride),
                 workspace="ch_hamming_topk_filtered_workspace", filt=filt)


def subcode_dist(q: torch.Tensor, g: torch.Tensor, idx: torch.Tensor, nbit: int, nsub: int, g_index_base: int = 0,
                 stream=None) -> torch.Tensor:
    """Per-sub-code distances of retrieved hits: idx [Qn, k] (as returned by hamming_topk / hamming_topk_masked on the same q, g and
    g_index_base) -> int32 [Qn, k, nsub], entry c = the distance inside bits [c nbit/nsub, (c+1) nbit/nsub); -1 rows where idx is -1.
    Reads idx back once to check it against the gallery (a synchronisation)."""
    lib = _lib.load()
    q, g = _check_packed(q, g)
    Qn, W = q.shape
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != Qn or idx.device != q.device:
        raise ValueError(f"idx must be an int64 tensor [{Qn}, k] on the queries' device")
    idx = idx.contiguous()
    k = idx.shape[1]
    out = torch.empty(Qn, k, int(nsub), dtype=torch.int32, device=q.device)
    with _dev_guard(q):
        _lib.check(lib.ch_hamming_subcode_dist(_lib.ptr(q), Qn, _lib.ptr(g), g.shape[0], W, _lib.ptr(idx), k, int(g_index_base),
                                               int(nbit), int(nsub), _lib.ptr(out), _lib.stream_ptr(stream)), "ch_hamming_subcode_dist")
    return out


def concept_mask(nbit: int, ncontext: int, concepts) -> torch.Tensor:
    """The shared mask [W] int64 (CPU) of a set of concepts: the code is concept-major, concept c owns bits
    [c nbit/ncontext, (c+1) nbit/ncontext) (models/arch/coop.py, csrc/head.hip).  Host arithmetic only.  An empty set gives the zero
    mask; a concept outside [0, ncontext) or named twice raises ValueError."""
    nbit, ncontext = int(nbit), int(ncontext)
    if nbit < 1 or ncontext < 1 or nbit % ncontext:
        raise ValueError(f"nbit = {nbit} is not a positive multiple of ncontext = {ncontext}")
    concepts = [int(c) for c in concepts]
    if any(c < 0 or c >= ncontext for c in concepts):
        raise ValueError(f"concepts {concepts} outside [0, {ncontext})")
    if len(set(concepts)) != len(concepts):
        raise ValueError(f"concepts {concepts} name a concept twice")
    sb = nbit // ncontext
    bits = 0
    for c in concepts:
        bits |= ((1 << sb) - 1) << (c * sb)
    W = (nbit + 63) // 64
    words = [(bits >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(W)]
    return torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in words], dtype=torch.int64)


def confidence_mask(codes: torch.Tensor, margin: float, stream=None) -> torch.Tensor:
    """[rows, nbit] fp32 codes -> [rows, W] int64: bit i is set iff |codes[:, i]| > margin -- the bits a query is sure of.  Two
    ch_pack_sign launches (codes > margin, -codes > margin) and an OR; bits past nbit stay zero."""
    return pack_sign(codes, margin, stream) | pack_sign(-codes, margin, stream)


def topk_merge(idx_lists: torch.Tensor, dist_lists: torch.Tensor, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """[nlists, Qn, k] per-shard lists -> global [Qn, k]."""
    lib = _lib.load()
    idx_lists = idx_lists.contiguous()
    dist_lists = dist_lists.contiguous()
    n, Qn, k = idx_lists.shape
    idx = torch.empty(Qn, k, dtype=torch.int64, device=idx_lists.device)
    dist = torch.empty(Qn, k, dtype=torch.int32, device=idx_lists.device)
    with _dev_guard(idx_lists):
        _lib.check(lib.ch_topk_merge(_lib.ptr(idx_lists), _lib.ptr(dist_lists), n, Qn, k, _lib.ptr(idx), _lib.ptr(dist),
                                     _lib.stream_ptr(stream)), "ch_topk_merge")
    return idx, dist


# ---------------------------------------------------------------------------------------------------------------
# labels
# ---------------------------------------------------------------------------------------------------------------
def labels_single(q_labels: torch.Tensor, g_labels: torch.Tensor) -> bool:
    """2-D indicator matrices whose rows all hold exactly one class (a gallery SHARD decides for its own rows only: the ranks of a
    sharded evaluation combine their answers, concepthash_amd.distributed)."""
    return bool(((q_labels != 0).sum(1) == 1).all().item()) and bool(((g_labels != 0).sum(1) == 1).all().item())


def prepare_labels(q_labels: torch.Tensor, g_labels: torch.Tensor, single=None):
    """Returns (q_lab, g_lab, LW).  1-D integer labels, or one-hot rows with exactly one class each -> int32 ids
    (LW = 0); otherwise multi-hot -> int64 bitmasks [rows, LW].  `single`: the decision, when the caller has made it (globally)."""
    if q_labels.dim() == 1 and g_labels.dim() == 1:
        return q_labels.to(torch.int32).contiguous(), g_labels.to(torch.int32).contiguous(), 0
    if q_labels.dim() != 2 or g_labels.dim() != 2 or q_labels.shape[1] != g_labels.shape[1]:
        raise ValueError("labels must both be 1-D class ids or 2-D [rows, C] indicator matrices")
    qb, gb = q_labels != 0, g_labels != 0
    if single is None:
        single = labels_single(q_labels, g_labels)
    if single:
        return qb.int().argmax(1).to(torch.int32).contiguous(), gb.int().argmax(1).to(torch.int32).contiguous(), 0
    C = qb.shape[1]
    LW = (C + 63) // 64

    def pack(b):
        pad = LW * 64 - C
        if pad:
            b = torch.cat([b, torch.zeros(b.shape[0], pad, dtype=torch.bool, device=b.device)], dim=1)
        w = torch.ones(64, dtype=torch.int64, device=b.device) << torch.arange(64, dtype=torch.int64, device=b.device)
        return (b.view(b.shape[0], LW, 64).to(torch.int64) * w).sum(-1).contiguous()  # wraps mod 2^64: bit 63 ok

    return pack(qb), pack(gb), LW


def map_seg_rows(Qn: int, G: int, W: int) -> int:
    """Gallery rows per segment of the two mAP passes (grid = query tiles x segments).  A workgroup holds its tile's counters in
    LDS -- (64 W + 1) x BLK x 4 B -- so an MI355X has 256 (x 2 at 64 bit) workgroup slots, and a launch takes
    ceil(workgroups / slots) rounds of one segment each: the segment count is chosen to fill whole rounds (e.g. NABirds size,
    97 tiles: 10 segments = 1.9 rounds instead of 11 = 2.1 -> 3) at about 1024 workgroups, segments of 256 .. 65,535 rows."""
    blk = 256 if W <= 2 else 128
    tiles = max(1, -(-Qn // blk))
    slots = 256 * max(1, (160 * 1024) // ((64 * W + 1) * blk * 4))
    nseg_max = max(1, min(65535, G // 256))          # segments of at least 256 rows
    nseg_min = max(1, -(-G // 65535))                # ... and at most 65,535 (16-bit counters)
    want = max(1, -(-1024 // tiles))
    hi = max(nseg_min, min(nseg_max, 2 * want))
    lo = min(hi, max(nseg_min, min(want, hi) // 2))
    best, best_cost = None, None
    for nseg in range(lo, hi + 1):
        rows = -(-G // nseg)
        cost = -(-(tiles * nseg) // slots) * (rows + 128)     # rounds x (rows of a segment + a workgroup's fixed cost in row units)
        if best_cost is None or cost < best_cost:
            best, best_cost = nseg, cost
    rows = -(-G // best)
    return int(min(65535, max(256, rows)))


def _hist_pass(q, g, seg_rows: int):
    """What both forms of mAP pass 1 start from: checked codes and the histogram [nseg, Qn, 64W+1, 2] int32 they fill."""
    q, g = _check_packed(q, g)
    Qn, W = q.shape
    G = g.shape[0]
    nseg = max(1, -(-G // seg_rows))
    # the pass writes every counter of every (segment, query); an empty gallery launches nothing
    return q, g, (torch.empty if G > 0 else torch.zeros)(nseg, Qn, 64 * W + 1, 2, dtype=torch.int32, device=q.device)


def hamming_hist(q, g, q_lab, g_lab, LW: int, seg_rows: int, stream=None) -> torch.Tensor:
    """mAP pass 1: [nseg, Qn, 64W+1, 2] int32 (uint32 bit patterns)."""
    lib = _lib.load()
    q, g, hist = _hist_pass(q, g, seg_rows)
    with _dev_guard(q):
        _lib.check(lib.ch_hamming_hist(_lib.ptr(q), q.shape[0], _lib.ptr(g), g.shape[0], q.shape[1], _lib.ptr(q_lab), _lib.ptr(g_lab), LW,
                                       seg_rows, _lib.ptr(hist), _lib.stream_ptr(stream)), "ch_hamming_hist")
    return hist


def hist_prefix(hist: torch.Tensor, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    hist = hist.contiguous()
    nseg, Qn, nb, _ = hist.shape
    base = torch.empty_like(hist)
    totals = torch.empty(Qn, 2, dtype=torch.int32, device=hist.device)
    with _dev_guard(hist):
        _lib.check(lib.ch_hamming_hist_prefix(_lib.ptr(hist), nseg, Qn, nb, _lib.ptr(base), _lib.ptr(totals),
                                              _lib.stream_ptr(stream)), "ch_hamming_hist_prefix")
    return base, totals


MAX_LIMITS = 16   # rank limits one AP pass accumulates (csrc/hamming.hip)


def _limit_chunks(limits: Sequence[int]):
    """(rows, C array, count) per launch of an entry that takes rank limits: MAX_LIMITS of them at a time; `rows` slices the [n, Qn]
    outputs."""
    lim = [int(r) for r in limits]
    for c0 in range(0, len(lim), MAX_LIMITS):
        chunk = lim[c0:c0 + MAX_LIMITS]
        yield slice(c0, c0 + len(chunk)), (ctypes.c_int64 * len(chunk))(*chunk), len(chunk)


def _ap(entry: str, q, g, q_lab, g_lab, LW: int, seg_rows: int, base: torch.Tensor, rank_limits: Sequence[int], first_rel, stream,
        operands=(), out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The calls of a ch_hamming_ap* entry on checked codes, one per MAX_LIMITS limits: S int64 / nrel int32 [n, Qn], zeroed here
    unless the caller hands them in as `out` (the entries accumulate); `operands` are the entry's own arguments, between base and the
    limits."""
    lib = _lib.load()
    q, g = _check_packed(q, g)
    Qn, W = q.shape
    n = len(rank_limits)
    S, nrel = out or (torch.zeros(n, Qn, dtype=torch.int64, device=q.device), torch.zeros(n, Qn, dtype=torch.int32, device=q.device))
    if first_rel is not None:
        first_rel = first_rel.to(torch.int32).contiguous()
    base = base.contiguous()
    with _dev_guard(q):
        for rows, arr, cnt in _limit_chunks(rank_limits):
            _lib.check(getattr(lib, entry)(_lib.ptr(q), Qn, _lib.ptr(g), g.shape[0], W, _lib.ptr(q_lab), _lib.ptr(g_lab), LW, seg_rows,
                                           _lib.ptr(base), *operands, arr, cnt, _lib.ptr(first_rel), _lib.ptr(S[rows]), _lib.ptr(nrel[rows]),
                                           _lib.stream_ptr(stream)), entry)
    return S, nrel


def hamming_ap(q, g, q_lab, g_lab, LW: int, seg_rows: int, base: torch.Tensor, rank_limit: int = -1,
               first_rel: Optional[torch.Tensor] = None, out_S: Optional[torch.Tensor] = None,
               out_nrel: Optional[torch.Tensor] = None, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """mAP pass 2 -> (S int64 [Qn] fixed-point numerators, nrel int32 [Qn]): `hamming_ap_multi` for one limit; out_S / out_nrel, where
    given, are accumulated into."""
    Qn = q.shape[0]
    S = out_S if out_S is not None else torch.zeros(Qn, dtype=torch.int64, device=q.device)
    nrel = out_nrel if out_nrel is not None else torch.zeros(Qn, dtype=torch.int32, device=q.device)
    _ap("ch_hamming_ap_multi", q, g, q_lab, g_lab, LW, seg_rows, base, [rank_limit], first_rel, stream, out=(S[None], nrel[None]))
    return S, nrel


def _relevance_of(idx: torch.Tensor, q_lab: torch.Tensor, g_lab_all: torch.Tensor, LW: int) -> torch.Tensor:
    """[Qn,k] bool relevance of retrieved rows (label gather; idx -1 -> False)."""
    safe = idx.clamp_min(0)
    if LW == 0:
        rel = g_lab_all[safe] == q_lab[:, None]
    else:
        rel = (g_lab_all[safe] & q_lab[:, None, :]).ne(0).any(-1)
    return rel & (idx >= 0)


def normalize_limits(limits: Sequence[int]):
    """-> (ascending unique limits with "unlimited" (<= 0) last as 0, index of every input limit in that list)"""
    norm = [int(r) if int(r) > 0 else 0 for r in limits]
    uniq = sorted({r for r in norm if r > 0}) + ([0] if 0 in norm else [])
    pos = {r: i for i, r in enumerate(uniq)}
    return uniq, [pos[r] for r in norm]


def hamming_ap_multi(q, g, q_lab, g_lab, LW: int, seg_rows: int, base: torch.Tensor, rank_limits: Sequence[int],
                     first_rel: Optional[torch.Tensor] = None, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """mAP pass 2 for a list of ascending rank limits (<= 0 = unlimited, last) in ONE gallery scan per 16 limits
    -> (S int64 [n, Qn], nrel int32 [n, Qn]); nrel[i] = number of relevant rows inside limit i."""
    return _ap("ch_hamming_ap_multi", q, g, q_lab, g_lab, LW, seg_rows, base, rank_limits, first_rel, stream)


def tie_bracket(bucket_counts: torch.Tensor, limits: Sequence[int], remove_first: bool = False, stream=None):
    """Smallest / largest AP over every order of the rows that share a distance ("tie bracket").
    bucket_counts: [Qn, 64W+1, 2] int32 -- rows / relevant rows per (query, distance) over the whole gallery, i.e. the histogram of
    hamming_hist / hamming_hist_rec summed over its segments (and shards).  limits: ascending, <= 0 = unlimited, last (normalize_limits).
    -> (S_low int64 [n, Qn], nrel_low int32 [n, Qn], S_high, nrel_high): AP = ap_from_fixed(S, nrel)."""
    lib = _lib.load()
    if bucket_counts.dim() != 3 or bucket_counts.shape[2] != 2 or bucket_counts.dtype != torch.int32:
        raise TypeError("bucket_counts must be an int32 tensor [Qn, nb, 2]")
    bc = bucket_counts.contiguous()
    Qn, nb, _ = bc.shape
    n = len(limits)
    S_lo, S_hi = (torch.zeros(n, Qn, dtype=torch.int64, device=bc.device) for _ in range(2))
    n_lo, n_hi = (torch.zeros(n, Qn, dtype=torch.int32, device=bc.device) for _ in range(2))
    with _dev_guard(bc):
        for rows, arr, cnt in _limit_chunks(limits):
            _lib.check(lib.ch_hamming_tie_bracket(_lib.ptr(bc), Qn, nb, arr, cnt, int(bool(remove_first)), _lib.ptr(S_lo[rows]),
                                                  _lib.ptr(n_lo[rows]), _lib.ptr(S_hi[rows]), _lib.ptr(n_hi[rows]),
                                                  _lib.stream_ptr(stream)), "ch_hamming_tie_bracket")
    return S_lo, n_lo, S_hi, n_hi


def tie_hits(bucket_counts: torch.Tensor, ks: Sequence[int], remove_first: bool = False) -> dict:
    """Bracket of hits@k (relevant rows in the top k), P@k and R@k over the tie orders: the two extreme numbers of relevant rows of
    the bucket that k cuts.  A few elementwise launches on [Qn, nb] integers.  With remove_first the dropped row is any row of the
    lowest non-empty bucket: hits and R@k (whose denominator loses a dropped relevant row) take their extremes over both kinds."""
    bc = bucket_counts.to(torch.int64)
    Qn, dev = bc.shape[0], bc.device
    ks = [int(k) for k in ks]

    def extremes(b):
        n, r = b[..., 0], b[..., 1]
        before = n.cumsum(1) - n
        lo, hi = [], []
        for k in ks:
            take = torch.minimum((k - before).clamp_min(0), n)
            hi.append(torch.minimum(r, take).sum(1))
            lo.append((take - (n - r)).clamp_min(0).sum(1))
        z = torch.zeros(Qn, 0, dtype=torch.int64, device=dev)
        return (torch.stack(lo, 1) if ks else z), (torch.stack(hi, 1) if ks else z), r.sum(1)

    def recall(h, tot):
        return torch.where(tot[:, None] > 0, h.double() / tot.clamp_min(1).double()[:, None], torch.zeros_like(h, dtype=torch.float64))

    if not remove_first or Qn == 0:
        lo, hi, tot = extremes(bc)
        rlo, rhi = recall(lo, tot), recall(hi, tot)
    else:
        nz = bc[..., 0] > 0
        rows = torch.arange(Qn, device=dev)
        d0 = nz.to(torch.int8).argmax(1)                       # the lowest non-empty bucket (first maximum)
        n0, r0 = bc[rows, d0, 0], bc[rows, d0, 1]
        can_irr, can_rel = n0 > r0, r0 > 0
        b_irr, b_rel = bc.clone(), bc.clone()
        b_irr[rows, d0, 0] -= can_irr.to(torch.int64)
        b_rel[rows, d0, 0] -= can_rel.to(torch.int64)
        b_rel[rows, d0, 1] -= can_rel.to(torch.int64)
        lo_i, hi_i, tot_i = extremes(b_irr)
        lo_r, hi_r, tot_r = extremes(b_rel)
        only_i, only_r = (~can_rel)[:, None], (~can_irr)[:, None]   # a query with no row at all: both walks see the same zeros
        lo = torch.where(only_i, lo_i, torch.where(only_r, lo_r, torch.minimum(lo_i, lo_r)))
        hi = torch.where(only_i, hi_i, torch.where(only_r, hi_r, torch.maximum(hi_i, hi_r)))
        rl_i, rl_r, rh_i, rh_r = recall(lo_i, tot_i), recall(lo_r, tot_r), recall(hi_i, tot_i), recall(hi_r, tot_r)
        rlo = torch.where(only_i, rl_i, torch.where(only_r, rl_r, torch.minimum(rl_i, rl_r)))
        rhi = torch.where(only_i, rh_i, torch.where(only_r, rh_r, torch.maximum(rh_i, rh_r)))
    out = dict(hits_low=lo.to(torch.int32), hits_high=hi.to(torch.int32))
    if not Qn or not ks:
        z = [0.0] * len(ks)
        out.update(precisions_low=z, precisions_high=list(z), recalls_low=list(z), recalls_high=list(z))
        return out
    kf = torch.tensor(ks, dtype=torch.float64, device=dev)
    vals = torch.stack([(lo.double() / kf).mean(0), (hi.double() / kf).mean(0), rlo.mean(0), rhi.mean(0)]).tolist()
    out.update(precisions_low=vals[0], precisions_high=vals[1], recalls_low=vals[2], recalls_high=vals[3])
    return out


def parse_limits(R, ks: Sequence[int]):
    """The R (an int, or a list or tuple of them) and ks of an evaluation -> (Rs, ks, many): lists of ints, and whether R was a list, i.e.
    whether mAP / S / nrel / ap come back as lists.  k < 1: ValueError."""
    ks = [int(k) for k in ks]
    if any(k <= 0 for k in ks):
        raise ValueError("P@k / R@k need k >= 1")
    many = isinstance(R, (list, tuple))
    return ([int(r) for r in R] if many else [int(R)]), ks, many


def pick_limits(x, idx_of, nR: int, many: bool):
    """The rows of a per-limit result x (`normalize_limits`' idx_of) that belong to the R: a list of them, or the one of a scalar R."""
    return [x[idx_of[i]] for i in range(nR)] if many else x[idx_of[0]]


def result_dict(sm: dict, S, nrel, total, idx_of, nR: int, many: bool) -> dict:
    """The keys every evaluation returns, from `summarize`'s statistics and the integers of the AP pass."""
    return dict(precisions=sm["precisions"], recalls=sm["recalls"], hits=sm["hits"], total=total, mAP=sm["mAPs"] if many else sm["mAPs"][0],
                S=pick_limits(S, idx_of, nR, many), nrel=pick_limits(nrel, idx_of, nR, many), ap=sm["aps"] if many else sm["aps"][0])


TIE_KEYS = ("mAP_low", "mAP_high", "ap_low", "ap_high", "S_low", "S_high", "nrel_low", "nrel_high", "precisions_low", "precisions_high",
            "recalls_low", "recalls_high", "hits_low", "hits_high")


def tie_results(bucket_counts: torch.Tensor, Rs: Sequence[int], ks: Sequence[int], remove_first: bool, many: bool,
                skip_queries_without_relevant: bool = False) -> dict:
    """The TIE_KEYS of evaluate(tie_bracket=True) from the whole-gallery bucket counts [Qn, nb, 2] (one kernel launch per 16 R)."""
    limits, idx_of = normalize_limits(Rs)
    S_lo, n_lo, S_hi, n_hi = tie_bracket(bucket_counts, limits, remove_first)
    Qn = bucket_counts.shape[0]
    total = torch.zeros(Qn, dtype=torch.int32, device=bucket_counts.device)      # no k here: summarize() uses it for R@k only
    lo = summarize(S_lo, n_lo, total, idx_of, Rs, [], skip_queries_without_relevant)
    hi = summarize(S_hi, n_hi, total, idx_of, Rs, [], skip_queries_without_relevant)
    pick = lambda x: pick_limits(x, idx_of, len(Rs), many)
    first = (lambda x: x) if many else (lambda x: x[0])
    out = dict(mAP_low=first(lo["mAPs"]), mAP_high=first(hi["mAPs"]), ap_low=first(lo["aps"]), ap_high=first(hi["aps"]),
               S_low=pick(S_lo), S_high=pick(S_hi), nrel_low=pick(n_lo), nrel_high=pick(n_hi))
    out.update(tie_hits(bucket_counts, ks, remove_first))
    return out


def tie_expected(bucket_counts: torch.Tensor, limits: Sequence[int], ks: Sequence[int] = (), remove_first: bool = False, stream=None):
    """Mean of AP@R, hits@k and R@k over every order of the rows that share a distance, every bucket uniformly permuted (DESIGN.md
    section 2.0, "tie expectation").  bucket_counts and limits as `tie_bracket` takes them; ks: depths >= 1, any order.
    -> (ap [n, Qn], hits [nk, Qn], recall [nk, Qn]), float64; one launch per 16 limits / 16 ks."""
    lib = _lib.load()
    if bucket_counts.dim() != 3 or bucket_counts.shape[2] != 2 or bucket_counts.dtype != torch.int32:
        raise TypeError("bucket_counts must be an int32 tensor [Qn, nb, 2]")
    ks = [int(k) for k in ks]
    if any(k <= 0 for k in ks):
        raise ValueError("P@k / R@k need k >= 1")
    bc = bucket_counts.contiguous()
    Qn, nb, _ = bc.shape
    ap = torch.zeros(len(limits), Qn, dtype=torch.float64, device=bc.device)
    hits, recall = (torch.zeros(len(ks), Qn, dtype=torch.float64, device=bc.device) for _ in range(2))
    if Qn == 0:
        return ap, hits, recall
    lim_chunks = list(_limit_chunks(limits))
    k_chunks = list(_limit_chunks(ks))      # the entry takes as many depths as limits: the same chunks of 16
    with _dev_guard(bc):
        for i in range(max(len(lim_chunks), len(k_chunks))):
            rows, arr, cnt = lim_chunks[i] if i < len(lim_chunks) else (None, None, 0)
            krows, karr, kcnt = k_chunks[i] if i < len(k_chunks) else (None, None, 0)
            _lib.check(lib.ch_hamming_tie_expected(_lib.ptr(bc), Qn, nb, arr, cnt, karr, kcnt, int(bool(remove_first)),
                                                   _lib.ptr(ap[rows]) if cnt else None, _lib.ptr(hits[krows]) if kcnt else None,
                                                   _lib.ptr(recall[krows]) if kcnt else None, _lib.stream_ptr(stream)),
                       "ch_hamming_tie_expected")
    return ap, hits, recall


EXPECTED_KEYS = ("mAP_expected", "ap_expected", "precisions_expected", "recalls_expected", "hits_expected")

EXPECTED_NEEDS_ALL_QUERIES = ("tie_expected with skip_queries_without_relevant=True: which queries have a relevant row inside R -- the set the "
                              "mean would run over -- itself depends on the tie order, so that mean is no per-query expectation; the tie "
                              "expectation is defined for the mean over all queries only")


def expected_results(bucket_counts: torch.Tensor, Rs: Sequence[int], ks: Sequence[int], remove_first: bool, many: bool) -> dict:
    """The EXPECTED_KEYS of evaluate(tie_expected=True) from the whole-gallery bucket counts [Qn, nb, 2]: mAP_expected (per R),
    ap_expected (float64 [Qn] per R), precisions_expected / recalls_expected (per k), hits_expected (float64 [Qn, nk]).  Means run over
    all queries."""
    limits, idx_of = normalize_limits(Rs)
    ap, hits, recall = tie_expected(bucket_counts, limits, ks, remove_first)
    Qn = bucket_counts.shape[0]
    aps = [ap[idx_of[i]] for i in range(len(Rs))]
    if Qn:
        kf = torch.tensor([float(k) for k in ks], dtype=torch.float64, device=ap.device)
        vals = torch.cat([ap.mean(1)[idx_of], (hits / kf[:, None]).mean(1), recall.mean(1)]).tolist()
    else:
        vals = [0.0] * (len(Rs) + 2 * len(ks))
    nR, nk = len(Rs), len(ks)
    return dict(mAP_expected=vals[:nR] if many else vals[0], ap_expected=aps if many else aps[0], precisions_expected=vals[nR:nR + nk],
                recalls_expected=vals[nR + nk:], hits_expected=hits.t().contiguous())


REC_BUDGET_BYTES = 4 << 30     # upper bound of the record buffer of one evaluation
REC_COMFORT_BYTES = 1 << 30    # ... and what is spent without need, for long lists (class-sorted galleries)


def record_cap(Qn: int, G: int, W: int, seg_rows: int) -> int:
    """Entries per (query, segment) record list of the one-scan form.  At least room for one relevant row in 64 of a segment (+ 32:
    any label distribution with no class above ~1.5 % of a segment fits), and as much more -- up to 2,048 entries -- as
    REC_COMFORT_BYTES buys: galleries listed class by class put a whole class (hundreds of rows) into one segment's lists.  Never
    above the segment length or REC_BUDGET_BYTES for the whole buffer.  A (tile, segment) workgroup whose lists overflow is redone
    by the two-scan kernel, so this only decides speed."""
    lib = _lib.load()
    wgs = int(lib.ch_hamming_rec_workgroups(Qn, G, W, seg_rows))
    unit = max(1, wgs * int(lib.ch_hamming_rec_block(W)) * 8)          # bytes per list entry over all lists
    cap = max(seg_rows // 64 + 32, min(2048, REC_COMFORT_BYTES // unit))
    return int(max(1, min(cap, seg_rows, REC_BUDGET_BYTES // unit)))


def records_fit(Qn: int, G: int, W: int, seg_rows: int) -> bool:
    """False where REC_BUDGET_BYTES cannot even hold the minimum list length (very large Qn x G): the lists would overflow nearly
    everywhere and the recording scan would be paid on top of the two-scan form -- evaluate() then runs the two-scan form."""
    return record_cap(Qn, G, W, seg_rows) >= min(seg_rows, seg_rows // 64 + 32)


OVERFLOW_SWITCH = 0.30     # predicted fraction of overflowing (query tile, segment) workgroups above which two scans are faster
OVERFLOW_MIN_PAIRS = 1 << 31   # below this many (query, row) pairs the whole evaluation is < 1 ms: not worth a prediction


def predicted_overflow(q_lab: torch.Tensor, g_lab: torch.Tensor, W: int, seg_rows: int, cap: int) -> float:
    """Fraction of the recording scan's (query tile, gallery segment) workgroups in which some query's record list would exceed
    `cap` entries -- EXACT for single-label ids, from the per-segment class histogram of the gallery labels (a few launches on
    G + Qn x nseg elements; one host read).  A list overflows when a query's class has more than `cap` rows inside one segment:
    galleries listed class by class under shuffled queries do that in nearly every workgroup, and there the one-scan form (which
    redoes every overflowed workgroup with the two-scan kernel) loses to running two scans outright: 81 vs 65 ms at 16,384 x 1M x
    128 bit."""
    lib = _lib.load()
    G, Qn = g_lab.shape[0], q_lab.shape[0]
    if G == 0 or Qn == 0 or cap >= seg_rows:
        return 0.0
    nseg = -(-G // seg_rows)
    blk = int(lib.ch_hamming_rec_block(W))
    ncls = int(torch.maximum(q_lab.max(), g_lab.max()).item()) + 1
    seg_id = torch.arange(G, device=g_lab.device, dtype=torch.int64) // seg_rows
    counts = torch.bincount(seg_id * ncls + g_lab.to(torch.int64), minlength=nseg * ncls).view(nseg, ncls)
    over = counts[:, q_lab.to(torch.int64)] > cap                               # [nseg, Qn]
    pad = (-Qn) % blk
    if pad:
        over = torch.cat([over, torch.zeros(nseg, pad, dtype=torch.bool, device=over.device)], dim=1)
    return float(over.view(nseg, -1, blk).any(dim=2).float().mean().item())


def hamming_hist_rec(q, g, q_lab, g_lab, LW: int, seg_rows: int, rec_cap: Optional[int] = None, stream=None):
    """mAP pass 1 of the one-scan form: the histogram of hamming_hist plus the per-lane record lists of the relevant rows
    -> (hist, records) where records = (rec, rec_cap, rec_cnt, wg_flags) is what hamming_ap_rec takes."""
    lib = _lib.load()
    q, g, hist = _hist_pass(q, g, seg_rows)
    Qn, W = q.shape
    G = g.shape[0]
    cap = int(rec_cap) if rec_cap else record_cap(Qn, G, W, seg_rows)
    wgs = int(lib.ch_hamming_rec_workgroups(Qn, G, W, seg_rows))
    blk = int(lib.ch_hamming_rec_block(W))
    rec = torch.empty(max(1, wgs) * cap * blk, 2, dtype=torch.int32, device=q.device)
    rec_cnt = torch.empty(hist.shape[0], Qn, dtype=torch.int32, device=q.device)
    wg_flags = torch.zeros(max(1, wgs), dtype=torch.int32, device=q.device)
    with _dev_guard(q):
        _lib.check(lib.ch_hamming_hist_rec(_lib.ptr(q), Qn, _lib.ptr(g), G, W, _lib.ptr(q_lab), _lib.ptr(g_lab), LW, seg_rows,
                                           _lib.ptr(hist), _lib.ptr(rec), cap, _lib.ptr(rec_cnt), _lib.ptr(wg_flags),
                                           _lib.stream_ptr(stream)), "ch_hamming_hist_rec")
    return hist, (rec, cap, rec_cnt, wg_flags)


def hamming_ap_rec(q, g, q_lab, g_lab, LW: int, seg_rows: int, base: torch.Tensor, records, rank_limits: Sequence[int],
                   first_rel: Optional[torch.Tensor] = None, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """hamming_ap_multi from the records of hamming_hist_rec (no second distance scan except for overflowed workgroups)."""
    rec, cap, rec_cnt, wg_flags = records
    return _ap("ch_hamming_ap_rec", q, g, q_lab, g_lab, LW, seg_rows, base, rank_limits, first_rel, stream,
               (_lib.ptr(rec), cap, _lib.ptr(rec_cnt), _lib.ptr(wg_flags)))


# ---------------------------------------------------------------------------------------------------------------
# ranked lists of any depth and hash lookup (csrc/hamming_rank.hip)
# ---------------------------------------------------------------------------------------------------------------
RANK_BUDGET_BYTES = 1 << 30    # hist + base of one chunk of queries (the budget `record_cap` spends on its lists)


def _u32(t: torch.Tensor) -> torch.Tensor:
    """non-negative integers < 2^32 -> int32 holding their uint32 bit patterns"""
    t = t.to(torch.int64)
    return torch.where(t >= (1 << 31), t - (1 << 32), t).to(torch.int32)


def bucket_counts(q: torch.Tensor, g: torch.Tensor, seg_rows: Optional[int] = None, stream=None):
    """The histogram pass without labels -> (hist [nseg, Qn, 64W+1, 2], base (same shape: `hist_prefix`), counts int64 [Qn, 64W+1]):
    counts[i, d] = gallery rows at distance d of query i.  The pass takes labels; it is handed zeros (every row "relevant"), and
    column 0 of its pairs is the row count.  seg_rows: default `map_seg_rows`."""
    q, g = _check_packed(q, g)
    Qn, W = q.shape
    G = g.shape[0]
    seg = int(seg_rows) if seg_rows else map_seg_rows(Qn, G, W)
    zq = torch.zeros(Qn, dtype=torch.int32, device=q.device)
    zg = torch.zeros(G, dtype=torch.int32, device=q.device)
    hist = hamming_hist(q, g, zq, zg, 0, seg, stream=stream)
    base, _ = hist_prefix(hist, stream=stream)
    return hist, base, hist[..., 0].sum(0, dtype=torch.int64)


def rank_scatter(q, g, seg_rows: int, base: torch.Tensor, out_start: torch.Tensor, out_limit: torch.Tensor, out_idx: torch.Tensor,
                 out_dist: torch.Tensor, g_index_base: int = 0, stream=None, check: bool = True) -> None:
    """ch_hamming_rank_scatter: row j of query i, of 0-based rank r in ascending (distance, index), goes to slot out_start[i] + r of the
    flat out_idx (int64) / out_dist (int32) when r < out_limit[i].  base: `bucket_counts(q, g, seg_rows)[1]`.  The limits must fit the
    buffers: out_start[i] + out_limit[i] <= out_idx.numel() (checked here, a host read; `check=False` is for callers whose limits fit by
    construction)."""
    lib = _lib.load()
    q, g = _check_packed(q, g)
    Qn, W = q.shape
    G = g.shape[0]
    nseg = max(1, -(-G // seg_rows))
    if tuple(base.shape) != (nseg, Qn, 64 * W + 1, 2) or base.dtype != torch.int32 or not base.is_contiguous():
        raise ValueError(f"base must be a contiguous int32 tensor [{nseg}, {Qn}, {64 * W + 1}, 2], got {base.dtype} {tuple(base.shape)}")
    if out_idx.dtype != torch.int64 or out_dist.dtype != torch.int32 or not out_idx.is_contiguous() or not out_dist.is_contiguous() \
            or out_idx.numel() != out_dist.numel():
        raise ValueError("out_idx (int64) and out_dist (int32) must be contiguous and of one size")
    start = out_start.to(torch.int64).contiguous()
    limit = out_limit.to(torch.int64)
    if start.shape != (Qn,) or limit.shape != (Qn,):
        raise ValueError(f"out_start and out_limit must be [{Qn}]")
    if check and Qn and (bool((start < 0).any()) or bool((limit < 0).any()) or int((start + limit).max()) > out_idx.numel()):
        raise ValueError("out_start / out_limit reach outside the output buffers")
    if out_idx.numel() == 0 or Qn == 0 or G == 0:
        return                               # no slot to fill (every limit is 0): nothing to launch, and an empty tensor has no address
    limit = _u32(limit).contiguous()
    with _dev_guard(q):
        _lib.check(lib.ch_hamming_rank_scatter(_lib.ptr(q), Qn, _lib.ptr(g), G, W, int(seg_rows), _lib.ptr(base), _lib.ptr(start),
                                               _lib.ptr(limit), int(g_index_base), _lib.ptr(out_idx), _lib.ptr(out_dist),
                                               _lib.stream_ptr(stream)), "ch_hamming_rank_scatter")


def _ranked_inputs(q, g, mask, radius):
    q, g = _check_packed(q, g)
    Qn, W = q.shape
    if mask is not None:
        if mask.dim() == 2:
            raise ValueError("a per-query mask [Qn, W] is not built for ranked lists / radius search (both passes would need the mask); "
                             "pass one shared int64 [W] mask, or rank with hamming_topk_masked (k <= 128)")
        mask, _ = _check_mask(mask, Qn, W, q.device, "queries")
        q, g = q & mask[None, :], g & mask[None, :]          # popcount((q ^ g) & m) = popcount((q & m) ^ (g & m))
    if radius is not None and not 0 <= int(radius) <= 64 * W:
        raise ValueError(f"radius must be in [0, {64 * W}], got {radius}")
    return q, g


def _query_chunks(Qn: int, G: int, W: int, seg_rows: Optional[int]):
    """(c0, c1, seg_rows) blocks of queries whose hist + base stay under RANK_BUDGET_BYTES"""
    c0 = 0
    while c0 < Qn:
        n = Qn - c0
        while True:
            seg = int(seg_rows) if seg_rows else map_seg_rows(n, G, W)
            per_query = 2 * max(1, -(-G // seg)) * (64 * W + 1) * 8
            fit = max(1, RANK_BUDGET_BYTES // per_query)
            if n <= fit:
                break
            n = fit
        yield c0, c0 + n, seg
        c0 += n


def hamming_ranked(q: torch.Tensor, g: torch.Tensor, k: int, g_index_base: int = 0, radius: Optional[int] = None,
                   mask: Optional[torch.Tensor] = None, seg_rows: Optional[int] = None, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first k rows of every query's ranking by ascending (distance, gallery index), for ANY k >= 1 (hamming_topk stops at 128):
    (idx int64 [Qn, k], dist int32 [Qn, k]), -1 past min(k, G) -- with `radius`, -1 past the rows with dist <= radius.  Histogram pass,
    prefix, then the pass that writes every row out at its rank (csrc/hamming_rank.hip).  mask: one shared int64 [W] mask
    (dist = popcount((q ^ g) & mask)); a per-query mask is a ValueError.  Queries go in chunks that keep hist + base under 1 GiB."""
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    q, g = _ranked_inputs(q, g, mask, radius)
    Qn, W = q.shape
    G = g.shape[0]
    idx = torch.full((Qn, k), -1, dtype=torch.int64, device=q.device)
    dist = torch.full((Qn, k), -1, dtype=torch.int32, device=q.device)
    if Qn == 0 or G == 0:
        return idx, dist
    for c0, c1, seg in _query_chunks(Qn, G, W, seg_rows):
        qc = q[c0:c1]
        _, base, counts = bucket_counts(qc, g, seg, stream=stream)
        if radius is None:
            limit = torch.full((c1 - c0,), min(k, G), dtype=torch.int64, device=q.device)
        else:
            limit = counts[:, :int(radius) + 1].sum(1).clamp_max(k)
        start = torch.arange(c0, c1, dtype=torch.int64, device=q.device) * k
        rank_scatter(qc, g, seg, base, start, limit, idx.view(-1), dist.view(-1), g_index_base, stream=stream,
                     check=False)         # slots i k .. i k + limit_i - 1, limit_i <= k
    return idx, dist


def hamming_radius(q: torch.Tensor, g: torch.Tensor, radius: int, g_index_base: int = 0, mask: Optional[torch.Tensor] = None,
                   max_hits: Optional[int] = None, seg_rows: Optional[int] = None, stream=None):
    """Hash lookup: every gallery row within `radius` bits of each query, as CSR -> (offsets int64 [Qn + 1], idx int64 [total],
    dist int32 [total]); query i's rows are offsets[i]:offsets[i + 1], ascending (distance, gallery index), at most `max_hits` of them
    when given.  radius outside [0, 64 W]: ValueError.  mask as in `hamming_ranked`.  Reads the list lengths back (a synchronisation)."""
    if radius is None:
        raise ValueError("hamming_radius needs a radius")
    if max_hits is not None and int(max_hits) < 0:
        raise ValueError(f"max_hits must be >= 0, got {max_hits}")
    q, g = _ranked_inputs(q, g, mask, radius)
    Qn, W = q.shape
    G = g.shape[0]
    dev = q.device
    offsets = torch.zeros(Qn + 1, dtype=torch.int64, device=dev)
    idxs, dists = [], []
    if Qn and G:
        done = 0
        for c0, c1, seg in _query_chunks(Qn, G, W, seg_rows):
            qc = q[c0:c1]
            _, base, counts = bucket_counts(qc, g, seg, stream=stream)
            limit = counts[:, :int(radius) + 1].sum(1)
            if max_hits is not None:
                limit = limit.clamp_max(int(max_hits))
            ends = limit.cumsum(0)
            total = int(ends[-1])
            idx = torch.full((total,), -1, dtype=torch.int64, device=dev)
            dist = torch.full((total,), -1, dtype=torch.int32, device=dev)
            rank_scatter(qc, g, seg, base, ends - limit, limit, idx, dist, g_index_base, stream=stream,
                         check=False)     # the lists tile [0, total)
            offsets[c0 + 1:c1 + 1] = ends + done
            done += total
            idxs.append(idx)
            dists.append(dist)
    if len(idxs) == 1:
        return offsets, idxs[0], dists[0]
    if not idxs:
        return offsets, torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    return offsets, torch.cat(idxs), torch.cat(dists)


LOOKUP_KEYS = ("precisions_radius", "recalls_radius", "retrieved_radius", "empty_radius", "lookup_retrieved", "lookup_hits")


def lowest_bucket(counts2: torch.Tensor) -> torch.Tensor:
    """[Qn, nb, 2] -> [Qn] int64: every query's lowest non-empty distance bucket (0 for a query with no row at all)"""
    return (counts2[..., 0] != 0).to(torch.int8).argmax(1)


def hash_lookup_stats(counts2: torch.Tensor, radii: Sequence[int], first=None) -> dict:
    """Hash lookup within a Hamming radius ("P@H<=r") from the whole-gallery bucket counts [Qn, nb, 2] (rows /
    relevant rows per (query, distance): the histogram of the mAP passes summed over its segments).  Pure torch, CPU or GPU.  Per
    radius r and query: retrieved = sum_{d<=r} rows, hits = sum_{d<=r} relevant rows, P = hits / retrieved (0 where nothing is
    retrieved), R = hits / total relevant (0 where the query has no relevant row).
    first = (d0 [Qn], first_rel [Qn]): remove_first_retrieved -- the dropped rank-1 row lies in the query's lowest non-empty bucket d0
    (`lowest_bucket`) and is relevant where first_rel is 1: retrieved and hits lose it for every r >= d0, and the recall denominator
    loses a dropped relevant row, as R@k's does.
    -> lookup_retrieved, lookup_hits int64 [Qn, len(radii)]; precisions_radius, recalls_radius, retrieved_radius (mean rows retrieved)
    and empty_radius (share of queries that retrieve nothing): lists of floats, one per radius."""
    if counts2.dim() != 3 or counts2.shape[2] != 2:
        raise TypeError("counts2 must be an integer tensor [Qn, nb, 2]")
    Qn, nb, _ = counts2.shape
    radii = [int(r) for r in radii]
    if any(r < 0 or r >= nb for r in radii):
        raise ValueError(f"radii must be in [0, {nb - 1}], got {radii}")
    c = counts2.to(torch.int64)
    if counts2.dtype == torch.int32:
        c = c & 0xFFFFFFFF                                  # uint32 bit patterns
    dev = c.device
    rad = torch.tensor(radii, dtype=torch.int64, device=dev)
    cn, cr = c[..., 0].cumsum(1), c[..., 1].cumsum(1)
    retrieved, hits = cn[:, rad], cr[:, rad]
    total = cr[:, -1] if nb else torch.zeros(Qn, dtype=torch.int64, device=dev)
    if first is not None:
        d0, first_rel = first
        d0, first_rel = d0.to(dev, torch.int64), first_rel.to(dev, torch.int64)
        dropped = ((d0[:, None] <= rad[None, :]) & (cn[:, -1] > 0)[:, None]).to(torch.int64)
        retrieved = retrieved - dropped
        hits = hits - first_rel[:, None] * dropped
        total = total - first_rel * (cn[:, -1] > 0).to(torch.int64)
    out = dict(lookup_retrieved=retrieved, lookup_hits=hits)
    if not Qn or not radii:
        z = [0.0] * len(radii)
        out.update(precisions_radius=z, recalls_radius=list(z), retrieved_radius=list(z), empty_radius=list(z))
        return out
    zero = torch.zeros(retrieved.shape, dtype=torch.float64, device=dev)
    P = torch.where(retrieved > 0, hits.double() / retrieved.clamp_min(1).double(), zero)
    R = torch.where(total[:, None] > 0, hits.double() / total.clamp_min(1).double()[:, None], zero)
    vals = torch.stack([P.mean(0), R.mean(0), retrieved.double().mean(0), (retrieved == 0).double().mean(0)]).tolist()
    out.update(precisions_radius=vals[0], recalls_radius=vals[1], retrieved_radius=vals[2], empty_radius=vals[3])
    return out


def ap_from_fixed(S: torch.Tensor, nrel: torch.Tensor) -> torch.Tensor:
    """AP[q] = S / (nrel * 2^32) in float64 (0 where nrel == 0); S holds uint64 bit patterns."""
    Sf = S.to(torch.float64)
    Sf = torch.where(S < 0, Sf + 18446744073709551616.0, Sf)
    n = nrel.to(torch.float64)
    return torch.where(nrel > 0, Sf / (n.clamp_min(1.0) * TWO32), torch.zeros_like(Sf))


def summarize(S, nrel, total, idx_of, Rs: Sequence[int], ks: Sequence[int], skip_queries_without_relevant: bool = False) -> dict:
    """Host-side statistics from the per-limit integers of one multi-limit AP pass: limits were Rs + ks (idx_of maps each to
    its row of S / nrel).  mAP per R; P@k = hits / k and R@k = hits / total with hits = nrel under limit k.
    skip_queries_without_relevant: the ONE convention of the AP definition that changes numbers ("Retrieval
    definition"): a query with no relevant row inside its top R has AP = 0.  False (default): it counts in the
    mean with that 0.  True (the HashNet / OrthoHash-family convention, `if tsum == 0: continue`): it is left out of the mean --
    mAP@R = mean of AP over the queries that have a relevant row in their top R (0.0 when no query has one).  Identical whenever
    every query has a relevant row inside R, e.g. mAP@all on CUB-200 / Cars196 / NABirds."""
    Qn = total.shape[0]
    dev = total.device
    nR = len(Rs)
    aps = [ap_from_fixed(S[idx_of[i]], nrel[idx_of[i]]) for i in range(nR)]
    hits = torch.zeros(Qn, len(ks), dtype=torch.int32, device=dev)
    if not Qn:
        return dict(mAPs=[0.0] * nR, aps=aps, hits=hits, precisions=[0.0] * len(ks), recalls=[0.0] * len(ks))
    if skip_queries_without_relevant:
        means = []
        for i, a in enumerate(aps):
            has = nrel[idx_of[i]] > 0
            means.append(a.sum() / has.sum().clamp_min(1).double())    # a is 0 where nrel == 0
    else:
        means = [a.mean() for a in aps]                     # 0-dim float64 tensors; ONE device->host copy for all of them below
    tot = total.clamp_min(1).double()
    for t, k in enumerate(ks):
        h = nrel[idx_of[nR + t]]
        hits[:, t] = h
        means.append((h.double() / k).mean())
    for t in range(len(ks)):
        h = hits[:, t]
        means.append(torch.where(total > 0, h.double() / tot, torch.zeros_like(tot)).mean())
    vals = torch.stack(means).tolist()
    return dict(mAPs=vals[:nR], aps=aps, hits=hits, precisions=vals[nR:nR + len(ks)], recalls=vals[nR + len(ks):])


def use_records(ops, Qn: int, rows: int, W: int, LW: int, seg_rows: int, q_lab, g_lab, records: Optional[bool] = None,
                rec_cap: Optional[int] = None) -> bool:
    """Whether an evaluation whose scan walks `rows` gallery rows takes the record (one-scan) form.  An explicit `records` wins;
    `ops` without `hamming_hist_rec` have the two-scan form only; otherwise CH_HAMMING_RECORDS=0 turns it off, and it needs lists
    that fit (`records_fit`, or the caller's `rec_cap`).  The label layout then decides which form is faster (never the result): left
    to the default capacity, a large single-label problem whose lists would overflow almost everywhere runs two scans."""
    if records is not None:
        return bool(records)
    if not hasattr(ops, "hamming_hist_rec") or os.environ.get("CH_HAMMING_RECORDS", "1") == "0" \
            or (rec_cap is None and not records_fit(Qn, rows, W, seg_rows)):
        return False
    if rec_cap is None and LW == 0 and Qn * rows >= OVERFLOW_MIN_PAIRS:
        return predicted_overflow(q_lab, g_lab, W, seg_rows, record_cap(Qn, rows, W, seg_rows)) <= OVERFLOW_SWITCH
    return True


def empty_result(Qn: int, W: int, dev, Rs: Sequence[int], ks: Sequence[int], many: bool, tie_bracket: bool, radii,
                 tie_expected: bool = False) -> dict:
    """What the evaluation returns without a query or without a gallery row: zeros in every key's type and shape."""
    z64 = torch.zeros(Qn, dtype=torch.int64, device=dev)
    z32 = torch.zeros(Qn, dtype=torch.int32, device=dev)
    out = dict(mAP=0.0, precisions=[0.0] * len(ks), recalls=[0.0] * len(ks), S=z64, nrel=z32,
               hits=torch.zeros(Qn, len(ks), dtype=torch.int32, device=dev), total=z32, ap=z64.double())
    if many:
        out.update(mAP=[0.0] * len(Rs), S=[z64] * len(Rs), nrel=[z32] * len(Rs), ap=[z64.double()] * len(Rs))
    if tie_bracket:
        for side in ("low", "high"):
            out.update({"mAP_" + side: out["mAP"], "ap_" + side: out["ap"], "S_" + side: out["S"], "nrel_" + side: out["nrel"],
                        "precisions_" + side: list(out["precisions"]), "recalls_" + side: list(out["recalls"]),
                        "hits_" + side: out["hits"]})
    if tie_expected:
        out.update(mAP_expected=out["mAP"], ap_expected=out["ap"], precisions_expected=list(out["precisions"]),
                   recalls_expected=list(out["recalls"]), hits_expected=torch.zeros(Qn, len(ks), dtype=torch.float64, device=dev))
    if radii is not None:
        out.update(hash_lookup_stats(torch.zeros(Qn, 64 * W + 1, 2, dtype=torch.int32, device=dev), radii))
    return out


class WholeGallery:
    """The gallery side of `evaluate_gallery` for a gallery this process holds whole: nothing is exchanged.
    (`distributed.ShardedRetrieval` is the row-sharded one.)  gallery / labels: the rows this process scans; rows: the WHOLE gallery's
    row count; scan_rows: the longest scan of any process, which sizes the segments and the record lists."""

    def __init__(self, gallery: torch.Tensor, labels: torch.Tensor, ops):
        self.gallery, self.labels, self.ops = gallery, labels, ops
        self.rows = self.scan_rows = gallery.shape[0]

    def first_relevant(self, q, q_lab, g_lab, LW: int) -> torch.Tensor:
        """int32 [Qn]: is every query's rank-1 row relevant"""
        idx, _ = self.ops.hamming_topk(q, self.gallery, 1)
        return _relevance_of(idx, q_lab, g_lab, LW)[:, 0].to(torch.int32)

    def bases(self, hist: torch.Tensor, want_counts: bool):
        """this process's histogram -> ("ranked before" bases of its segments, whole-gallery totals [Qn, 2], whole-gallery bucket
        counts [Qn, nb, 2] or None)"""
        base, totals = self.ops.hist_prefix(hist)
        return base, totals, hist.sum(0, dtype=hist.dtype) if want_counts else None

    def reduce(self, S: torch.Tensor, nrel: torch.Tensor) -> None:
        """this process's AP integers -> the whole gallery's, in place"""


def evaluate_gallery(gal, q: torch.Tensor, q_labels: torch.Tensor, R=-1, ks: Sequence[int] = (1, 5, 10), remove_first: bool = False,
                     seg_rows: Optional[int] = None, records: Optional[bool] = None, rec_cap: Optional[int] = None,
                     skip_queries_without_relevant: bool = False, tie_bracket: bool = False,
                     radii: Optional[Sequence[int]] = None, single: Optional[bool] = None, tie_expected: bool = False) -> dict:
    """The evaluation behind `evaluate` and `ShardedRetrieval.evaluate`: labels, rank-1 relevance, histogram pass (with records or
    without), prefix, ONE AP pass over every R and k, the statistics.  `gal` (`WholeGallery` or a `ShardedRetrieval`) holds the rows
    this process scans, the `ops` that scan them and the steps that cross ranks; every process of a sharded evaluation gets here with
    the same q and takes the same path through this body.  single: `prepare_labels`' decision, where the caller has made it."""
    if tie_expected and skip_queries_without_relevant:
        raise ValueError(EXPECTED_NEEDS_ALL_QUERIES)
    ops, g = gal.ops, gal.gallery
    dev = q.device
    Qn, W = q.shape
    ql, gl = q_labels.to(dev), gal.labels.to(dev)
    q_lab, g_lab, LW = ops.prepare_labels(ql, gl, single)
    Rs, ks, many = parse_limits(R, ks)
    if Qn == 0 or gal.rows == 0:
        return empty_result(Qn, W, dev, Rs, ks, many, tie_bracket, radii, tie_expected)
    # relevance of every query's rank-1 row (the self-match when the test set is the database)
    first_rel = gal.first_relevant(q, q_lab, g_lab, LW) if remove_first else None
    seg = seg_rows or ops.map_seg_rows(Qn, gal.scan_rows, W)
    limits, idx_of = ops.normalize_limits(Rs + ks)
    # one distance scan (histogram + records of the relevant rows, prefix, the AP terms from the records) or two
    rec = use_records(ops, Qn, gal.scan_rows, W, LW, seg, q_lab, g_lab, records, rec_cap)
    hist, recs = ops.hamming_hist_rec(q, g, q_lab, g_lab, LW, seg, rec_cap=rec_cap) if rec else (ops.hamming_hist(q, g, q_lab, g_lab, LW, seg), None)
    base, totals, counts2 = gal.bases(hist, tie_bracket or tie_expected or radii is not None)
    if rec:
        S, nrel = ops.hamming_ap_rec(q, g, q_lab, g_lab, LW, seg, base, recs, limits, first_rel=first_rel)
    else:
        S, nrel = ops.hamming_ap_multi(q, g, q_lab, g_lab, LW, seg, base, limits, first_rel=first_rel)
    gal.reduce(S, nrel)
    total = totals[:, 1].clone()
    if remove_first:
        total = total - first_rel
    sm = ops.summarize(S, nrel, total, idx_of, Rs, ks, skip_queries_without_relevant)
    out = result_dict(sm, S, nrel, total, idx_of, len(Rs), many)
    if tie_bracket:
        out.update(ops.tie_results(counts2, Rs, ks, remove_first, many, skip_queries_without_relevant))
    if tie_expected:     # from the integers every process holds alike: the same bits under any sharding
        out.update(ops.expected_results(counts2, Rs, ks, remove_first, many))
    if radii is not None:
        out.update(hash_lookup_stats(counts2, radii, (lowest_bucket(counts2), first_rel) if remove_first else None))
    return out


def evaluate(q: torch.Tensor, g: torch.Tensor, q_labels: torch.Tensor, g_labels: torch.Tensor, R=-1,
             ks: Sequence[int] = (1, 5, 10), remove_first: bool = False, seg_rows: Optional[int] = None,
             records: Optional[bool] = None, rec_cap: Optional[int] = None, skip_queries_without_relevant: bool = False,
             tie_bracket: bool = False, radii: Optional[Sequence[int]] = None, tie_expected: bool = False) -> dict:
    """Single-GPU mAP@R + P@k + R@k on packed codes: histogram pass, prefix, ONE AP pass whose rank limits are R (an int or
    a list) and every k -- the number of relevant rows inside limit k is exactly hits@k, for any k.  Returns python
    floats/lists plus the raw integer statistics (S, nrel, hits, total) that the parity tests compare bit-for-bit with the
    oracle.  With a list R: mAP, S, nrel, ap are lists (one entry per R).
    records (default on; CH_HAMMING_RECORDS=0 = off): the one-scan form -- the histogram pass also records the relevant rows and
    the AP pass walks those records instead of scanning the gallery again; rec_cap overrides the list capacity (tests).  Left to the
    default, large single-label problems first predict (exactly, from the labels) how many workgroups' lists would overflow and run
    the two-scan form where most would (`predicted_overflow`).
    skip_queries_without_relevant: which queries the mean of AP runs over (`summarize`); the integers S / nrel do not depend on it.
    tie_bracket: also report, for every statistic, the smallest and the largest value any order of equal-distance rows can give
    (TIE_KEYS: mAP_low / mAP_high ... hits_low / hits_high) -- one more small kernel on the histogram this
    call holds anyway.  Off: exactly the keys, integers and launches of before.
    tie_expected: also report the MEAN of every statistic over the tie orders, every bucket uniformly permuted (EXPECTED_KEYS:
    mAP_expected, ap_expected, precisions_expected, recalls_expected, hits_expected) -- the value that depends on no
    sort, inside the bracket; one more small kernel on the same histogram, with or without tie_bracket.  The means run over all queries:
    together with skip_queries_without_relevant it is a ValueError.
    radii: a list of Hamming radii adds the hash-lookup statistics of `hash_lookup_stats` (LOOKUP_KEYS) from the same histogram -- a few
    elementwise launches; None adds nothing and costs nothing."""
    q, g = _check_packed(q, g)
    return evaluate_gallery(WholeGallery(g, g_labels, sys.modules[__name__]), q, q_labels, R, ks, remove_first, seg_rows, records, rec_cap,
                            skip_queries_without_relevant, tie_bracket, radii, tie_expected=tie_expected)


# ---------------------------------------------------------------------------------------------------------------
# evaluation by rank counting: ONE pipeline (collect, sort, count, AP) under the weighted (asymmetric) distance
# (csrc/hamming_rankcount.hip), the ternary one (csrc/hamming_ternary.hip) and the dense ones (csrc/dense_rank.hip); the sections
# below hold what each of those rankings supplies to it
# ---------------------------------------------------------------------------------------------------------------
RANK_LIST_MAX = 8192   # longest list of relevant keys a workgroup of the rank-count scan holds in LDS (csrc/hamming_shared.h)


def rank_seg_rows(Qn: int, G: int) -> int:
    """Gallery rows per segment of the rank-count scan (grid = queries x segments): about 2,048 workgroups, segments of at least 256
    rows, at most 65,535 of them."""
    want = max(1, -(-2048 // max(1, Qn)))
    return int(max(256, -(-G // want), -(-G // 65535)))


def _check_weighted(q: torch.Tensor, planes: torch.Tensor, g: torch.Tensor):
    q, g = _check_packed(q, g)
    Qn, W = q.shape
    if planes.dtype != torch.int64 or planes.device != q.device or planes.dim() != 3 or planes.shape[0] != Qn or planes.shape[2] != W \
            or planes.shape[1] not in WEIGHT_BITS:
        raise ValueError(f"planes must be an int64 tensor [{Qn}, 4 or 8, {W}] on the queries' device, got {planes.dtype} "
                         f"{tuple(planes.shape)} on {planes.device}")
    return q, planes.contiguous(), g


def _collect_pass(entry: str, operands, Qn: int, G: int, dev, q_lab, g_lab, LW: int, g_index_base: int, stream):
    """The collect pass of a ranking on checked operands -> (offsets int64 [Qn + 1], keys int64 [total], UNSORTED inside a slice, longest
    slice).  Two launches of the ch_*_rank_collect `entry` (count, then write) around the prefix; reads the total and the longest slice
    back (one synchronisation).  `operands` are the entry's own arguments, in front of the labels."""
    lib = _lib.load()
    count = torch.zeros(Qn, dtype=torch.int32, device=dev)
    offsets = torch.zeros(Qn + 1, dtype=torch.int64, device=dev)
    if Qn == 0 or G == 0:
        return offsets, torch.empty(0, dtype=torch.int64, device=dev), 0

    def call(off, keys):
        _lib.check(getattr(lib, entry)(*operands, _lib.ptr(q_lab), _lib.ptr(g_lab), LW, int(g_index_base), _lib.ptr(off), _lib.ptr(count),
                                       _lib.ptr(keys), _lib.stream_ptr(stream)), entry)

    with _dev_guard(count):
        call(None, None)
        offsets[1:] = count.cumsum(0, dtype=torch.int64)
        total, longest = torch.stack([offsets[-1], count.max().to(torch.int64)]).tolist()
        keys = torch.empty(total, dtype=torch.int64, device=dev)
        if total:
            count.zero_()
            call(offsets, keys)
    return offsets, keys, int(longest)


def _count_pass(entry: str, operands, Qn: int, G: int, dev, offsets, keys, list_cap: int, seg_rows, g_index_base: int, bins, stream):
    """The count pass of a ranking on checked operands: the Qn x G scan of the ch_*_rank_count `entry` -> bins int32 [total] (uint32 bit
    patterns); `bins`, where given, is added into (gallery shards).  `operands` are the entry's own arguments, in front of g_index_base."""
    lib = _lib.load()
    if bins is None:
        bins = torch.zeros(keys.numel(), dtype=torch.int32, device=dev)
    if Qn == 0 or G == 0 or keys.numel() == 0:
        return bins
    seg = int(seg_rows) if seg_rows else rank_seg_rows(Qn, G)
    with _dev_guard(bins):
        _lib.check(getattr(lib, entry)(*operands, int(g_index_base), seg, _lib.ptr(offsets), _lib.ptr(keys), int(list_cap), _lib.ptr(bins),
                                       _lib.stream_ptr(stream)), entry)
    return bins


def sort_slices(offsets: torch.Tensor, keys: torch.Tensor, wide: bool = False) -> torch.Tensor:
    """Every CSR slice of `keys` ascending AS UINT64.  Keys below 2^48 (a distance below 2^16 over a 32-bit index; `wide` = False says
    so) order alike as int64, and up to 32,767 slices the slice number fits above them: ONE sort of slice << 48 | key.  Keys that use all
    64 bits (`wide`: the dense ones), or more slices: flipping the top bit maps uint64 order onto int64 order -- harmless for small
    keys --; one sort of the flat buffer, then a stable sort by slice."""
    if keys.numel() == 0:
        return keys
    n = offsets[1:] - offsets[:-1]
    owner = torch.repeat_interleave(torch.arange(n.numel(), device=keys.device), n, output_size=keys.numel())
    if not wide and n.numel() <= 0x7FFF:
        return (torch.sort(keys | (owner << 48))[0] & ((1 << 48) - 1)).contiguous()
    top = -(1 << 63)
    flipped, order = torch.sort(keys ^ top)
    return (flipped[torch.sort(owner[order], stable=True)[1]] ^ top).contiguous()


def sort_slices_unsigned(offsets: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
    """`sort_slices` of keys that use all 64 bits (int64 holding uint64 bit patterns)."""
    return sort_slices(offsets, keys, wide=True)


def rank_ap(offsets: torch.Tensor, bins: torch.Tensor, rank_limits: Sequence[int], remove_first: bool = False, stream=None):
    """AP integers from the bins, one launch per MAX_LIMITS limits -> (S int64 [n, Qn], nrel int32 [n, Qn], total int32 [Qn]) in the
    layout of `hamming_ap_multi`; total = a query's relevant rows (less a dropped relevant rank-1 row)."""
    lib = _lib.load()
    Qn = offsets.numel() - 1
    n = len(rank_limits)
    dev = offsets.device
    S = torch.zeros(n, Qn, dtype=torch.int64, device=dev)
    nrel = torch.zeros(n, Qn, dtype=torch.int32, device=dev)
    total = torch.zeros(Qn, dtype=torch.int32, device=dev)
    if Qn == 0:
        return S, nrel, total
    with _dev_guard(offsets):
        for rows, arr, cnt in _limit_chunks(rank_limits):
            _lib.check(lib.ch_hamming_rank_ap(Qn, _lib.ptr(offsets), _lib.ptr(bins) if bins.numel() else _lib.ptr(None), arr, cnt,
                                              int(bool(remove_first)), _lib.ptr(S[rows]), _lib.ptr(nrel[rows]), _lib.ptr(total),
                                              _lib.stream_ptr(stream)), "ch_hamming_rank_ap")
    return S, nrel, total


def _evaluate_by_rank_counting(Qn: int, G: int, W: int, dev, operands, collect, count, wide: bool, q_labels, g_labels, R, ks,
                               remove_first: bool, skip_queries_without_relevant: bool, seg_rows, list_cap) -> dict:
    """The evaluation behind `evaluate_weighted`, `evaluate_ternary` and `evaluate_dense`, which have checked their arguments: the keys
    of each query's relevant rows are collected and sorted, one Qn x G scan counts how many gallery rows fall between consecutive ones,
    and one lane per query turns the counts into ranks and AP terms (`rank_ap`; more than 16 limits repeat that last launch only).
    What describes the ranking: Qn, G, the device, the W that `empty_result` wants; `operands()` -> the scan operands, prepared only
    once there is something to scan; its two passes, collect(*operands, q_lab, g_lab, LW) and count(*operands, offsets, keys, list_cap,
    seg_rows); `wide`: its keys use all 64 bits (`sort_slices`)."""
    Rs, ks, many = parse_limits(R, ks)
    if Qn == 0 or G == 0:
        return empty_result(Qn, W, dev, Rs, ks, many, False, None)
    ops = operands()
    q_lab, g_lab, LW = prepare_labels(q_labels.to(dev), g_labels.to(dev))
    limits, idx_of = normalize_limits(Rs + ks)
    offsets, keys, longest = collect(*ops, q_lab, g_lab, LW)
    keys = sort_slices(offsets, keys, wide)
    cap = int(list_cap) if list_cap else max(1, min(RANK_LIST_MAX, longest))
    bins = count(*ops, offsets, keys, cap, seg_rows)
    S, nrel, total = rank_ap(offsets, bins, limits, remove_first)
    sm = summarize(S, nrel, total, idx_of, Rs, ks, skip_queries_without_relevant)
    return result_dict(sm, S, nrel, total, idx_of, len(Rs), many)


# ---------------------------------------------------------------------------------------------------------------
# ... under the weighted (asymmetric) distance (csrc/hamming_rankcount.hip)
# ---------------------------------------------------------------------------------------------------------------
def rank_collect(q: torch.Tensor, planes: torch.Tensor, g: torch.Tensor, q_lab: torch.Tensor, g_lab: torch.Tensor, LW: int,
                 g_index_base: int = 0, stream=None):
    """The keys D << 32 | global index of every query's relevant rows, as CSR -> (offsets int64 [Qn + 1], keys int64 [total], UNSORTED
    inside a slice, longest slice).  Two ch_hamming_rank_collect launches (count, then write) around the prefix; reads the total and the
    longest slice back (one synchronisation).  q_lab / g_lab / LW: `prepare_labels`."""
    q, planes, g = _check_weighted(q, planes, g)
    Qn, W = q.shape
    G = g.shape[0]
    return _collect_pass("ch_hamming_rank_collect", (_lib.ptr(q), _lib.ptr(planes), planes.shape[1], Qn, _lib.ptr(g), G, W), Qn, G, q.device,
                         q_lab, g_lab, LW, g_index_base, stream)


def rank_count(q: torch.Tensor, planes: torch.Tensor, g: torch.Tensor, offsets: torch.Tensor, keys: torch.Tensor, list_cap: int,
               seg_rows: Optional[int] = None, g_index_base: int = 0, bins: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """The Qn x G scan -> bins int32 [total] (uint32 bit patterns): bins[offsets[i] + pos] = gallery rows with exactly pos of query i's
    relevant keys below their own key (rows above the largest relevant key are not counted).  keys: `sort_slices(rank_collect(...))`.
    `bins`, where given, is added into (gallery shards)."""
    q, planes, g = _check_weighted(q, planes, g)
    Qn, W = q.shape
    G = g.shape[0]
    return _count_pass("ch_hamming_rank_count", (_lib.ptr(q), _lib.ptr(planes), planes.shape[1], Qn, _lib.ptr(g), G, W), Qn, G, q.device,
                       offsets, keys, list_cap, seg_rows, g_index_base, bins, stream)


def evaluate_weighted(codes: torch.Tensor, g: torch.Tensor, q_labels: torch.Tensor, g_labels: torch.Tensor, bits: int = 8,
                      mask: Optional[torch.Tensor] = None, R=-1, ks: Sequence[int] = (1, 5, 10), remove_first: bool = False,
                      skip_queries_without_relevant: bool = False, seg_rows: Optional[int] = None,
                      list_cap: Optional[int] = None) -> dict:
    """`evaluate` under the weighted (asymmetric) ranking that `hamming_topk_weighted` serves: ascending
    (D, gallery index), D = sum_j w_ij [bit_j(q_i) != bit_j(g)] with the query's own |code| quantised to `bits` (4 or 8) bits as its
    weights.  codes: [Qn, nbit] fp32, the real-valued query codes (the queries are pack_sign(codes) and weight_planes(codes, bits,
    mask)); g: the packed gallery; mask as `weight_planes` takes it.  Returns the keys of `evaluate` -- mAP, precisions, recalls, hits,
    total, S, nrel, ap, lists under a list R -- with the same integers' meaning, exact for any R and k, by rank counting
    (`_evaluate_by_rank_counting`).  seg_rows / list_cap (tests): the scan's segmentation and the list length up to which a list is
    searched in LDS -- neither changes a result."""
    if codes.dim() != 2:
        raise ValueError("codes must be 2-D [Qn, nbit] real-valued query codes")
    if g.dtype != torch.int64 or g.dim() != 2:
        raise TypeError("the gallery must be a 2-D int64 tensor of packed codes")
    Qn, nbit = codes.shape
    W = (nbit + 63) // 64
    if g.shape[1] != W:
        raise ValueError(f"query codes of {nbit} bits take {W} words per code, the gallery has {g.shape[1]}")
    if int(bits) not in WEIGHT_BITS:
        raise ValueError(f"weight bits must be one of {WEIGHT_BITS}, got {bits}")

    def operands():
        c = codes.to(g.device, torch.float32).contiguous()
        return pack_sign(c), weight_planes(c, bits, mask)[0], g

    return _evaluate_by_rank_counting(Qn, g.shape[0], W, g.device, operands, rank_collect, rank_count, False, q_labels, g_labels, R, ks,
                                      remove_first, skip_queries_without_relevant, seg_rows, list_cap)


# ---------------------------------------------------------------------------------------------------------------
# ternary codes (csrc/hamming_ternary.hip; DESIGN.md section 2.0, "ternary codes")
# ---------------------------------------------------------------------------------------------------------------
def check_margin(margin, what: str = "margin") -> float:
    """A ternary margin: a finite number >= 0 (ValueError otherwise; None included -- there is no default, the scale of the codes
    belongs to the run)."""
    if margin is None:
        raise ValueError(f"{what} is required: ternary codes have no default margin (the scale of the codes belongs to the run)")
    m = float(margin)
    if not (m >= 0.0) or m == float("inf"):
        raise ValueError(f"{what} must be finite and >= 0, got {margin}")
    return m


def pack_ternary(codes: torch.Tensor, margin: float, stream=None) -> torch.Tensor:
    """[rows, nbit] fp32 -> [rows, 2, W] int64, the two adjacent bit planes of the ternary code t_j = sign(x_j) where |x_j| > margin,
    0 otherwise (NaN gives 0): plane 0 (sign) = pack_sign(codes) & mask, plane 1 (mask) = confidence_mask(codes, margin); bits past
    nbit are zero in both.  One launch.  The margin is compared as fp32."""
    lib = _lib.load()
    if codes.dim() != 2:
        raise ValueError("codes must be 2-D")
    margin = check_margin(margin)
    codes = codes.to(torch.float32).contiguous()
    rows, nbit = codes.shape
    out = torch.empty(rows, 2, (nbit + 63) // 64, dtype=torch.int64, device=codes.device)
    with _dev_guard(codes):
        _lib.check(lib.ch_pack_ternary(_lib.ptr(codes), rows, nbit, margin, _lib.ptr(out), _lib.stream_ptr(stream)), "ch_pack_ternary")
    return out


def _check_ternary(q3: torch.Tensor, g3: torch.Tensor, nbit: int):
    if q3.dtype != torch.int64 or g3.dtype != torch.int64 or q3.dim() != 3 or g3.dim() != 3 or q3.shape[1] != 2 or g3.shape[1] != 2:
        raise TypeError("ternary codes must be int64 tensors [rows, 2, W] (pack_ternary)")
    if q3.shape[2] != g3.shape[2]:
        raise ValueError(f"query has {q3.shape[2]} words per plane, gallery {g3.shape[2]}")
    if q3.device != g3.device:
        raise ValueError("query and gallery codes must be on the same device")
    W = q3.shape[2]
    if not 1 <= int(nbit) <= 64 * W:
        raise ValueError(f"nbit must be in [1, {64 * W}] for planes of {W} words, got {nbit}")
    return q3.contiguous(), g3.contiguous()


def ternary_dist(q3: torch.Tensor, g3: torch.Tensor, nbit: int, stream=None) -> torch.Tensor:
    """Full [Qn, G] int32 matrix of K = nbit - sum_j t_q,j t_g,j (small problems), in half bits: K / 2 is the distance in bits."""
    lib = _lib.load()
    q3, g3 = _check_ternary(q3, g3, nbit)
    out = torch.empty(q3.shape[0], g3.shape[0], dtype=torch.int32, device=q3.device)
    with _dev_guard(q3):
        _lib.check(lib.ch_ternary_dist(_lib.ptr(q3), q3.shape[0], _lib.ptr(g3), g3.shape[0], q3.shape[2], int(nbit), _lib.ptr(out),
                                       _lib.stream_ptr(stream)), "ch_ternary_dist")
    return out


def ternary_topk(q3: torch.Tensor, g3: torch.Tensor, nbit: int, k: int, g_index_base: int = 0, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k by ascending (K, gallery index) on `pack_ternary` codes: (idx int64 [Qn,k], dist int32 [Qn,k] = K); -1 where k > G.  Lists of
    gallery shards merge with `topk_merge`."""
    q3, g3 = _check_ternary(q3, g3, nbit)
    return _topk("ch_ternary_topk", q3, g3, int(k), g_index_base, stream, workspace="ch_ternary_topk_workspace", behind_w=(int(nbit),))


def ternary_topk_filtered(q3: torch.Tensor, g3: torch.Tensor, nbit: int, k: int, allow: Optional[torch.Tensor] = None,
                          group: Optional[torch.Tensor] = None, want: Optional[torch.Tensor] = None, exclude: bool = False,
                          g_index_base: int = 0, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`ternary_topk` among ADMITTED rows only; allow, group, want and exclude as `hamming_topk_filtered` takes them (a row of the
    two-plane gallery is one row of the bitmap and of the group plane)."""
    q3, g3 = _check_ternary(q3, g3, nbit)
    filt = _check_filter(allow, group, want, exclude, q3.shape[0], g3.shape[0], q3.device)
    return _topk("ch_ternary_topk_filtered", q3, g3, int(k), g_index_base, stream, workspace="ch_ternary_topk_filtered_workspace", filt=filt,
                 behind_w=(int(nbit),))


def ternary_rank_collect(q3: torch.Tensor, g3: torch.Tensor, nbit: int, q_lab: torch.Tensor, g_lab: torch.Tensor, LW: int,
                         g_index_base: int = 0, stream=None):
    """`rank_collect` under K: the keys K << 32 | global index of every query's relevant rows -> (offsets, keys, longest slice)."""
    q3, g3 = _check_ternary(q3, g3, nbit)
    Qn, _, W = q3.shape
    G = g3.shape[0]
    return _collect_pass("ch_ternary_rank_collect", (_lib.ptr(q3), Qn, _lib.ptr(g3), G, W, int(nbit)), Qn, G, q3.device, q_lab, g_lab, LW,
                         g_index_base, stream)


def ternary_rank_count(q3: torch.Tensor, g3: torch.Tensor, nbit: int, offsets: torch.Tensor, keys: torch.Tensor, list_cap: int,
                       seg_rows: Optional[int] = None, g_index_base: int = 0, bins: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """`rank_count` under K -> bins int32 [total]; keys: `sort_slices(ternary_rank_collect(...))`."""
    q3, g3 = _check_ternary(q3, g3, nbit)
    Qn, _, W = q3.shape
    G = g3.shape[0]
    return _count_pass("ch_ternary_rank_count", (_lib.ptr(q3), Qn, _lib.ptr(g3), G, W, int(nbit)), Qn, G, q3.device, offsets, keys, list_cap,
                       seg_rows, g_index_base, bins, stream)


def evaluate_ternary(q3: torch.Tensor, g3: torch.Tensor, nbit: int, q_labels: torch.Tensor, g_labels: torch.Tensor, R=-1,
                     ks: Sequence[int] = (1, 5, 10), remove_first: bool = False, skip_queries_without_relevant: bool = False,
                     seg_rows: Optional[int] = None, list_cap: Optional[int] = None) -> dict:
    """`evaluate` under the ternary ranking that `ternary_topk` serves: ascending (K, gallery index) on
    `pack_ternary` codes of both sides.  Returns the keys of `evaluate_weighted` -- mAP, precisions, recalls, hits, total, S, nrel, ap,
    lists under a list R -- exact for any R and k, by the same rank counting (`_evaluate_by_rank_counting`).  seg_rows / list_cap
    (tests) change no result."""
    q3, g3 = _check_ternary(q3, g3, nbit)
    return _evaluate_by_rank_counting(q3.shape[0], g3.shape[0], q3.shape[2], g3.device, lambda: (q3, g3, nbit), ternary_rank_collect,
                                      ternary_rank_count, False, q_labels, g_labels, R, ks, remove_first, skip_queries_without_relevant,
                                      seg_rows, list_cap)


# ---------------------------------------------------------------------------------------------------------------
# real-valued codes (csrc/dense_rank.hip; DESIGN.md section 2.0, "real-valued codes")
# ---------------------------------------------------------------------------------------------------------------
DENSE_METRICS = ("cosine", "euclidean", "dot")   # the position is the metric id of the C entries
DENSE_MAX_DIM = 256
DENSE_MAX_K = 128


def dense_metric_id(metric) -> int:
    if metric not in DENSE_METRICS:
        raise ValueError(f"metric must be one of {DENSE_METRICS}, got {metric!r}")
    return DENSE_METRICS.index(metric)


def check_dense_codes(codes, what: str = "codes") -> torch.Tensor:
    """Real-valued codes for a dense ranking: 2-D [rows, n], 1 <= n <= 256, every entry finite (ValueError otherwise: the kernels
    do not define the order of NaN or infinite distances).  -> fp32, contiguous, where it was."""
    codes = torch.as_tensor(codes)
    if codes.dim() != 2:
        raise ValueError(f"{what} must be 2-D [rows, n] real-valued codes")
    if not 1 <= codes.shape[1] <= DENSE_MAX_DIM:
        raise ValueError(f"{what} have {codes.shape[1]} dimensions; the dense rankings take 1 .. {DENSE_MAX_DIM}")
    codes = codes.to(torch.float32).contiguous()
    if codes.numel() and not bool(torch.isfinite(codes).all()):
        raise ValueError(f"{what} hold NaN or infinite entries: the dense rankings are defined on finite codes")
    return codes


class DenseCodes:
    """The scan operand of the dense entries (`prepare_dense`): `data`, fp32 in blocks of 64 rows, dimension-major inside a block
    (include/concepthash_hip.h), with the rows, dimensions and metric it was prepared for."""

    def __init__(self, data: torch.Tensor, rows: int, n: int, metric: str):
        self.data, self.rows, self.n, self.metric = data, int(rows), int(n), metric

    @property
    def device(self):
        return self.data.device


def prepare_dense(codes, metric: str, stream=None) -> DenseCodes:
    """[rows, n] real codes -> the operand of dense_dist / dense_topk / dense_rank_collect / dense_rank_count under `metric`: rows
    normalised once for "cosine" (a zero row stays zero), copied for the others.  Non-finite codes: ValueError, before any launch."""
    mid = dense_metric_id(metric)
    codes = check_dense_codes(codes)
    lib = _lib.load()
    rows, n = codes.shape
    out = torch.empty(int(lib.ch_dense_prepared_bytes(rows, n)) // 4, dtype=torch.float32, device=codes.device)
    with _dev_guard(codes):
        _lib.check(lib.ch_dense_prepare(_lib.ptr(codes), rows, n, mid, _lib.ptr(out), _lib.stream_ptr(stream)), "ch_dense_prepare")
    return DenseCodes(out, rows, n, metric)


def _check_dense_pair(q: DenseCodes, g: DenseCodes, metric=None) -> int:
    if not isinstance(q, DenseCodes) or not isinstance(g, DenseCodes):
        raise TypeError("dense rankings take prepare_dense(codes, metric) operands")
    if metric is not None and (dense_metric_id(metric), metric) != (dense_metric_id(q.metric), q.metric):
        raise ValueError(f"the queries were prepared for {q.metric!r}, not for {metric!r}")
    if q.metric != g.metric:
        raise ValueError(f"queries were prepared for {q.metric!r}, the gallery for {g.metric!r}")
    if q.n != g.n:
        raise ValueError(f"queries have {q.n} dimensions, the gallery {g.n}")
    if q.device != g.device:
        raise ValueError("query and gallery codes must be on the same device")
    return dense_metric_id(q.metric)


def dense_dist(q: DenseCodes, g: DenseCodes, metric: Optional[str] = None, stream=None) -> torch.Tensor:
    """Full [Qn, G] fp32 matrix of the distance (small problems), the bits every other dense entry ranks by.  metric: the operands'
    own where left out; another one is a ValueError (an operand is prepared for one metric)."""
    lib = _lib.load()
    mid = _check_dense_pair(q, g, metric)
    out = torch.empty(q.rows, g.rows, dtype=torch.float32, device=q.device)
    if q.rows and g.rows:
        with _dev_guard(q.data):
            _lib.check(lib.ch_dense_dist(_lib.ptr(q.data), q.rows, _lib.ptr(g.data), g.rows, q.n, mid, _lib.ptr(out),
                                         _lib.stream_ptr(stream)), "ch_dense_dist")
    return out


def dense_topk(q: DenseCodes, g: DenseCodes, metric: Optional[str], k: int, g_index_base: int = 0, seg_rows: Optional[int] = None,
               stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k by ascending (distance, gallery index) under `metric` (None: the operands' own; another one is a ValueError): (idx int64 [Qn,k], dist fp32 [Qn,k]); idx -1 and dist
    +inf where k > G.  1 <= k <= 128.  Lists of gallery shards merge exactly by ascending (`dense_order(dist)`, idx).  seg_rows
    (tests): the scan's segmentation -- it changes no result."""
    lib = _lib.load()
    mid = _check_dense_pair(q, g, metric)
    k = int(k)
    if not 1 <= k <= DENSE_MAX_K:
        raise ValueError(f"k must be in [1, {DENSE_MAX_K}], got {k}")
    Qn, G = q.rows, g.rows
    seg = int(seg_rows) if seg_rows else 0
    idx = torch.empty(Qn, k, dtype=torch.int64, device=q.device)
    dist = torch.empty(Qn, k, dtype=torch.float32, device=q.device)
    if Qn == 0:
        return idx, dist
    wsb = int(lib.ch_dense_topk_workspace(Qn, G, k, seg))
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    with _dev_guard(q.data):
        _lib.check(lib.ch_dense_topk(_lib.ptr(q.data), Qn, _lib.ptr(g.data) if G else _lib.ptr(None), G, q.n, mid, k, int(g_index_base),
                                     seg, _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(ws), wsb, _lib.stream_ptr(stream)), "ch_dense_topk")
    return idx, dist


def dense_order(dist: torch.Tensor) -> torch.Tensor:
    """ord(D) of fp32 distances as int64 in [0, 2^32): ascending as D ascends, -0 with +0 (the high word of a dense key)."""
    b = (dist.to(torch.float32) + 0.0).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(b >= (1 << 31), b ^ 0xFFFFFFFF, b ^ 0x80000000)


def dense_unorder(o: torch.Tensor) -> torch.Tensor:
    """The fp32 distance of an ord value (int64 in [0, 2^32)): the inverse of `dense_order`."""
    o = o.to(torch.int64) & 0xFFFFFFFF
    b = torch.where(o >= (1 << 31), o ^ 0x80000000, o ^ 0xFFFFFFFF)
    return torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32).view(torch.float32)


def dense_rank_collect(q: DenseCodes, g: DenseCodes, q_lab: torch.Tensor, g_lab: torch.Tensor, LW: int, g_index_base: int = 0, stream=None):
    """`rank_collect` under a dense metric: the keys ord(D) << 32 | global index of every query's relevant rows -> (offsets, keys,
    longest slice).  The keys use all 64 bits (int64 holding uint64 bit patterns): `sort_slices_unsigned` puts them in order."""
    mid = _check_dense_pair(q, g)
    return _collect_pass("ch_dense_rank_collect", (_lib.ptr(q.data), q.rows, _lib.ptr(g.data), g.rows, q.n, mid), q.rows, g.rows, q.device,
                         q_lab, g_lab, LW, g_index_base, stream)


def dense_rank_count(q: DenseCodes, g: DenseCodes, offsets: torch.Tensor, keys: torch.Tensor, list_cap: int, seg_rows: Optional[int] = None,
                     g_index_base: int = 0, bins: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """`rank_count` under a dense metric -> bins int32 [total]; keys: `sort_slices_unsigned(dense_rank_collect(...))`.  `bins`, where
    given, is added into (gallery shards)."""
    mid = _check_dense_pair(q, g)
    return _count_pass("ch_dense_rank_count", (_lib.ptr(q.data), q.rows, _lib.ptr(g.data), g.rows, q.n, mid), q.rows, g.rows, q.device,
                       offsets, keys, list_cap, seg_rows, g_index_base, bins, stream)


def evaluate_dense(q_codes, g_codes, q_labels: torch.Tensor, g_labels: torch.Tensor, metric: str, R=-1, ks: Sequence[int] = (1, 5, 10),
                   remove_first: bool = False, skip_queries_without_relevant: bool = False, seg_rows: Optional[int] = None,
                   list_cap: Optional[int] = None) -> dict:
    """`evaluate` under the ranking of the real-valued codes themselves: ascending (D, gallery index), D the
    cosine, squared Euclidean or negated dot distance of `metric` between [Qn, n] and [G, n] fp32 codes -- what `dense_topk` serves,
    and the upper end of the ladder Hamming < ternary / asymmetric < dense (mAP_dense - mAP is a run's quantisation gap).  Returns
    the keys of `evaluate_weighted` -- mAP, precisions, recalls, hits, total, S, nrel, ap, lists under a list R -- exact for any R and
    k under the fp32 distances of the kernels, by the same rank counting (`_evaluate_by_rank_counting`).  seg_rows / list_cap (tests)
    change no result."""
    dense_metric_id(metric)
    q_codes, g_codes = check_dense_codes(q_codes, "query codes"), check_dense_codes(g_codes, "gallery codes")
    if q_codes.shape[1] != g_codes.shape[1]:
        raise ValueError(f"queries have {q_codes.shape[1]} dimensions, the gallery {g_codes.shape[1]}")
    dev = g_codes.device
    return _evaluate_by_rank_counting(q_codes.shape[0], g_codes.shape[0], 1, dev,
                                      lambda: (prepare_dense(q_codes.to(dev), metric), prepare_dense(g_codes, metric)), dense_rank_collect,
                                      dense_rank_count, True, q_labels, g_labels, R, ks, remove_first, skip_queries_without_relevant,
                                      seg_rows, list_cap)


# ---------------------------------------------------------------------------------------------------------------
# two-stage search ("two-stage"): a Hamming shortlist, ordered by a dense distance
# ---------------------------------------------------------------------------------------------------------------
RERANK_MAX = 4096      # rows of a shortlist: their keys are sorted in 32 KB of LDS per query (csrc/dense_rank.hip)


def check_shortlist(k, shortlist) -> Tuple[int, int]:
    """(k, m) of a two-stage list: 1 <= k <= m <= 4096 (ValueError otherwise)"""
    k, m = int(k), int(shortlist)
    if not 1 <= m <= RERANK_MAX:
        raise ValueError(f"shortlist must be in [1, {RERANK_MAX}], got {m}")
    if not 1 <= k <= m:
        raise ValueError(f"k must be in [1, shortlist = {m}], got {k}")
    return k, m


def _check_rerank_codes(q_codes, g_codes, metric):
    mid = dense_metric_id(metric)
    q, g = check_dense_codes(q_codes, "query codes"), check_dense_codes(g_codes, "gallery codes")
    if q.shape[1] != g.shape[1]:
        raise ValueError(f"queries have {q.shape[1]} dimensions, the gallery {g.shape[1]}")
    if q.device != g.device:
        raise ValueError("query and gallery codes must be on the same device")
    return mid, q, g


def dense_rerank(q_codes, g_codes, cand: torch.Tensor, metric: str, k: int, g_index_base: int = 0, validate: bool = True,
                 stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The second stage: every query's candidate rows cand [Qn, m] (int64 global ids, row = id - g_index_base; a negative id is an
    empty slot) ordered by ascending (D, index) under `metric` and cut at k -> (idx int64 [Qn, k], dist fp32 [Qn, k]), -1 / +inf past
    the filled slots.  q_codes [Qn, n] and g_codes [G, n] are the RAW real-valued codes (`check_dense_codes`), not `prepare_dense`
    operands; D has the bits of `dense_dist` for the pair.  1 <= k <= m <= 4096.  A row listed twice appears twice.  validate: an id
    >= g_index_base + G is a ValueError before anything is launched (False: the caller vouches for the ids, e.g. `hamming_ranked`'s;
    the kernel treats such an id as an empty slot)."""
    mid, q, g = _check_rerank_codes(q_codes, g_codes, metric)
    cand = torch.as_tensor(cand)
    if cand.dtype != torch.int64 or cand.dim() != 2 or cand.shape[0] != q.shape[0]:
        raise ValueError(f"cand must be int64 [Qn = {q.shape[0]}, m] row ids, got {cand.dtype} {tuple(cand.shape)}")
    k, m = check_shortlist(k, cand.shape[1])
    Qn, G, base = q.shape[0], g.shape[0], int(g_index_base)
    if base < 0 or base + G > 1 << 32:
        raise ValueError(f"g_index_base = {base} with {G} rows: keys hold 32-bit row indices (0 <= g_index_base, g_index_base + G <= 2^32)")
    if cand.device != g.device:
        raise ValueError("cand and the codes must be on the same device")
    if validate and cand.numel() and int(cand.max()) >= base + G:
        raise ValueError(f"cand holds the id {int(cand.max())}, outside the gallery's [{base}, {base + G}) (negative ids are empty slots)")
    cand = cand.contiguous()
    idx = torch.empty(Qn, k, dtype=torch.int64, device=g.device)
    dist = torch.empty(Qn, k, dtype=torch.float32, device=g.device)
    if Qn == 0:
        return idx, dist
    lib = _lib.load()
    with _dev_guard(g):
        _lib.check(lib.ch_dense_rerank(_lib.ptr(q), Qn, _lib.ptr(g) if G else _lib.ptr(None), G, q.shape[1], mid, _lib.ptr(cand), m, k, base,
                                       _lib.ptr(idx), _lib.ptr(dist), _lib.stream_ptr(stream)), "ch_dense_rerank")
    return idx, dist


def rerank_topk(q_codes, g_codes, metric: str, k: int, shortlist: int, radius: Optional[int] = None, q_packed: Optional[torch.Tensor] = None,
                g_packed: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two-stage list: the first `shortlist` rows by ascending (Hamming distance, index) of the sign codes -- `hamming_ranked`, at
    every depth; with `radius`, only rows within that many bits -- ordered by ascending (D, index) under `metric` of the real-valued
    codes and cut at k -> (idx int64 [Qn, k], dist fp32 [Qn, k]), -1 / +inf past the filled slots.  q_packed / g_packed: the packed
    sign codes where the caller holds them (an index's); otherwise `pack_sign` of the codes.  1 <= k <= shortlist <= 4096."""
    k, m = check_shortlist(k, shortlist)
    _, q, g = _check_rerank_codes(q_codes, g_codes, metric)
    qp = pack_sign(q) if q_packed is None else q_packed
    gp = pack_sign(g) if g_packed is None else g_packed
    if qp.shape[0] != q.shape[0] or gp.shape[0] != g.shape[0]:
        raise ValueError(f"{qp.shape[0]} / {gp.shape[0]} packed codes for {q.shape[0]} / {g.shape[0]} real-valued codes")
    cand, _ = hamming_ranked(qp, gp, m, radius=radius)
    return dense_rerank(q, g, cand, metric, k, validate=False)


def _relevant_total(q_lab: torch.Tensor, g_lab: torch.Tensor, LW: int) -> torch.Tensor:
    """[Qn] int64: every query's relevant rows in the whole gallery (`prepare_labels` operands), a block of queries at a time"""
    Qn, G = q_lab.shape[0], g_lab.shape[0]
    out = torch.zeros(Qn, dtype=torch.int64, device=q_lab.device)
    step = max(1, (1 << 26) // max(G * max(LW, 1), 1))
    for c0 in range(0, Qn, step):
        qc = q_lab[c0:c0 + step]
        rel = g_lab[None, :] == qc[:, None] if LW == 0 else (g_lab[None, :, :] & qc[:, None, :]).ne(0).any(-1)
        out[c0:c0 + step] = rel.sum(1)
    return out


def evaluate_reranked(q_codes, g_codes, q_labels: torch.Tensor, g_labels: torch.Tensor, metric: str, shortlist: int, R=-1,
                      ks: Sequence[int] = (1, 5, 10), remove_first: bool = False, skip_queries_without_relevant: bool = False,
                      radius: Optional[int] = None, q_packed: Optional[torch.Tensor] = None, g_packed: Optional[torch.Tensor] = None) -> dict:
    """AP@R, P@k and R@k of the two-stage list of depth `shortlist` (`rerank_topk`) under the AP definition of `evaluate`: the keys of
    `evaluate_dense` -- mAP, precisions, recalls, hits, total (relevant rows of the WHOLE gallery: a relevant row the shortlist misses
    costs recall), S, nrel, ap, lists under a list R -- and
      R: the effective R (R = -1 means the shortlist), shortlist;
      agreement: {k: mean share of the exhaustive `dense_topk` top-k found in the two-stage top-k} for each k <= 128 of ks.
    R and every k must lie in [1, shortlist] (ValueError).  remove_first drops rank 1 of the final list.  The list arithmetic on
    [Qn, shortlist] is torch's; the lists are the kernels'."""
    Rs, ks, many = parse_limits(R, ks)
    _, m = check_shortlist(1, shortlist)
    Rs = [m if r == -1 else r for r in Rs]
    for what, vals in (("R", Rs), ("k", ks)):
        if any(not 1 <= v <= m for v in vals):
            raise ValueError(f"every {what} of a two-stage evaluation must lie in [1, shortlist = {m}] (R = -1: the shortlist), got {vals}")
    _, q, g = _check_rerank_codes(q_codes, g_codes, metric)
    dev = g.device
    q_lab, g_lab, LW = prepare_labels(torch.as_tensor(q_labels).to(dev), torch.as_tensor(g_labels).to(dev))
    if q_lab.shape[0] != q.shape[0] or g_lab.shape[0] != g.shape[0]:
        raise ValueError(f"{q_lab.shape[0]} / {g_lab.shape[0]} labels for {q.shape[0]} / {g.shape[0]} codes")
    idx, _ = rerank_topk(q, g, metric, m, m, radius, q_packed, g_packed)
    rel = _relevance_of(idx, q_lab, g_lab, LW)
    total = _relevant_total(q_lab, g_lab, LW)
    if remove_first:
        total = total - rel[:, 0].to(torch.int64)
        rel = rel[:, 1:]
    Qn, L = rel.shape
    seen = rel.to(torch.int64).cumsum(1)
    ranks = torch.arange(1, L + 1, dtype=torch.int64, device=dev)
    terms = torch.where(rel, torch.div(seen << 32, ranks[None, :], rounding_mode="floor"), torch.zeros_like(seen))   # floor(relrank 2^32 / rank)
    limits, idx_of = normalize_limits(Rs + ks)
    S = torch.stack([terms[:, :lim].sum(1) for lim in limits]) if limits else torch.zeros(0, Qn, dtype=torch.int64, device=dev)
    nrel = torch.stack([rel[:, :lim].sum(1).to(torch.int32) for lim in limits]) if limits else torch.zeros(0, Qn, dtype=torch.int32, device=dev)
    total = total.to(torch.int32)
    out = result_dict(summarize(S, nrel, total, idx_of, Rs, ks, skip_queries_without_relevant), S, nrel, total, idx_of, len(Rs), many)
    out.update(R=Rs if many else Rs[0], shortlist=m, agreement={})
    deep = [k for k in ks if k <= DENSE_MAX_K]
    if deep and Qn:
        full, _ = dense_topk(prepare_dense(q, metric), prepare_dense(g, metric), metric, max(deep))
        shares = []
        for k in deep:
            want = full[:, :k]
            found = ((want[:, :, None] == idx[:, None, :k]).any(-1) & (want >= 0)).sum(1).double()
            shares.append((found / (want >= 0).sum(1).clamp_min(1).double()).mean())
        out["agreement"] = dict(zip(deep, torch.stack(shares).tolist()))
    return out


# ---------------------------------------------------------------------------------------------------------------
# learned rotation: iterative quantisation of the real-valued codes ("learned rotation"; csrc/itq.hip)
# ---------------------------------------------------------------------------------------------------------------
ITQ_MAX_DIM = 256
ITQ_MAX_SEG = 4096


def check_blocks(n: int, blocks) -> int:
    """`blocks` of a block-diagonal rotation of n-dimensional codes: an int >= 1 that divides n (ValueError otherwise) -> block size s"""
    if isinstance(blocks, bool) or not isinstance(blocks, int):
        raise ValueError(f"blocks must be an int, got {blocks!r}")
    if blocks < 1 or n % blocks:
        raise ValueError(f"blocks = {blocks} does not divide the {n} dimensions of the codes (a rotation has n / blocks columns per block)")
    return n // blocks


def compact_rotation(R: torch.Tensor, blocks: int) -> torch.Tensor:
    """[n, n] block-diagonal -> [n, s], s = n / blocks: row b s + l holds R_b[l, :] (the form the kernels take).  An entry outside the
    blocks that is not zero is a ValueError."""
    n = R.shape[0]
    s = check_blocks(n, blocks)
    if tuple(R.shape) != (n, n):
        raise ValueError(f"a full rotation must be square, got {tuple(R.shape)}")
    diag = torch.arange(blocks, device=R.device)
    out = R.reshape(blocks, s, blocks, s)[diag, :, diag, :].reshape(n, s).contiguous()      # [blocks, s, s]
    if not torch.equal(full_rotation(out, blocks), R):
        raise ValueError(f"R is not block-diagonal under blocks = {blocks}: an entry outside the blocks is not zero")
    return out


def full_rotation(Rc: torch.Tensor, blocks: int) -> torch.Tensor:
    """[n, s] compact -> [n, n] block-diagonal"""
    n, s = Rc.shape
    return torch.block_diag(*Rc.reshape(blocks, s, s).unbind(0)).contiguous()


def _check_itq(codes, R, blocks):
    """The argument checks of itq_step / rotate_codes, all in front of the first launch -> (codes, compact R, n, s)"""
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.float32:
        raise TypeError(f"codes must be a float32 tensor, got {getattr(codes, 'dtype', type(codes))}")
    if codes.dim() != 2:
        raise ValueError(f"codes must be 2-D [rows, n] real-valued codes, got {tuple(codes.shape)}")
    n = codes.shape[1]
    if not 1 <= n <= ITQ_MAX_DIM:
        raise ValueError(f"codes have {n} dimensions; a learned rotation takes 1 .. {ITQ_MAX_DIM}")
    s = check_blocks(n, blocks)
    if R is not None:
        if not isinstance(R, torch.Tensor) or R.dtype != torch.float32:
            raise TypeError(f"R must be a float32 tensor, got {getattr(R, 'dtype', type(R))}")
        if R.dim() != 2 or tuple(R.shape) not in ((n, n), (n, s)):
            raise ValueError(f"R must be [{n}, {n}] (block-diagonal) or [{n}, {s}] (compact) for blocks = {blocks}, got {tuple(R.shape)}")
        if R.device != codes.device:
            raise ValueError("R and the codes must be on the same device")
        if not bool(torch.isfinite(R).all()):
            raise ValueError("R holds NaN or infinite entries")
        if tuple(R.shape) != (n, s):
            R = compact_rotation(R, blocks)
        R = R.contiguous()
    if codes.numel() and not bool(torch.isfinite(codes).all()):
        raise ValueError("codes hold NaN or infinite entries: a rotation is fitted on finite codes")
    return codes.contiguous(), R, n, s


def itq_step(codes: torch.Tensor, R: torch.Tensor, blocks: int, seg_rows: Optional[int] = None, stream=None):
    """One pass of iterative quantisation under the rotation R ([n, n] block-diagonal or [n, n / blocks] compact), the kernels' own
    fmaf chain and sign rule -> (M [n, s] float64: row j = sum_i sign(z_ij) codes[i, block of j], l1 = sum |z|, qerr = mean_i (1 -
    |z_i|_1 / (sqrt(n) |z_i|_2)), a zero row counting 1).  seg_rows (1 .. 4096; tests): rows whose M is accumulated in fp32 before the
    fp64 sum over segments.  No rows: zeros, l1 = 0, qerr = 0."""
    codes, Rc, n, s = _check_itq(codes, R, blocks)
    if R is None:
        raise TypeError("R must be a float32 tensor, got None")
    seg = 0 if seg_rows is None else int(seg_rows)
    if not 0 <= seg <= ITQ_MAX_SEG or (seg_rows is not None and seg < 1):
        raise ValueError(f"seg_rows must be in [1, {ITQ_MAX_SEG}], got {seg_rows!r}")
    return _itq_step(codes, Rc, n, s, seg, stream)


def _itq_step(codes, Rc, n: int, s: int, seg: int, stream=None):
    """`itq_step` behind its argument checks"""
    guard = _dev_guard(codes)
    lib = _lib.load()
    rows = codes.shape[0]
    M = torch.zeros(n, s, dtype=torch.float64, device=codes.device)
    if rows == 0:
        return M, 0.0, 0.0
    stats = torch.zeros(2, dtype=torch.float64, device=codes.device)
    wsb = int(lib.ch_itq_step_workspace(rows, n, s, seg))
    ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device=codes.device)
    with guard:
        _lib.check(lib.ch_itq_step(_lib.ptr(codes), rows, n, _lib.ptr(Rc), s, seg, _lib.ptr(M), _lib.ptr(stats), _lib.ptr(ws), ws.numel() * 8,
                                   _lib.stream_ptr(stream)), "ch_itq_step")
    l1, cs = stats.tolist()
    return M, l1, 1.0 - cs / rows


def rotate_codes(codes: torch.Tensor, R: torch.Tensor, blocks: int, stream=None) -> torch.Tensor:
    """[rows, n] fp32 -> codes R, entry by entry the fmaf chain of `itq_step` (a row rotates to the same bits alone or in a batch)"""
    codes, Rc, n, s = _check_itq(codes, R, blocks)
    if R is None:
        raise TypeError("R must be a float32 tensor, got None")
    guard = _dev_guard(codes)
    lib = _lib.load()
    out = torch.empty_like(codes)
    if codes.shape[0]:
        with guard:
            _lib.check(lib.ch_itq_rotate(_lib.ptr(codes), codes.shape[0], n, _lib.ptr(Rc), s, _lib.ptr(out), _lib.stream_ptr(stream)),
                       "ch_itq_rotate")
    return out


def procrustes_update(M: torch.Tensor, blocks: int) -> torch.Tensor:
    """M [n, s] float64 (`itq_step`) -> the next rotation, compact [n, s] float64: per block M_b = U S W^T (fp64 SVD on the host) and
    R_b = W U^T, the maximiser of tr(R_b M_b) over orthogonal matrices -- the orthogonal Procrustes solution."""
    n, s = M.shape
    U, _, Wh = torch.linalg.svd(M.detach().to("cpu", torch.float64).reshape(blocks, s, s))
    return (U @ Wh).transpose(1, 2).reshape(n, s)


def fit_rotation(codes: torch.Tensor, blocks: int, iters: int = 50, tol: float = 1e-6) -> dict:
    """Fit a block-diagonal rotation to `codes` [G, n] fp32 by iterative quantisation from R_0 = I: pass t scores R_t (`itq_step`) and,
    unless it is the last, builds R_{t+1} (`procrustes_update`); at most `iters` updates, and none after a pass whose gain
    l1_t - l1_{t-1} is <= tol l1_{t-1}.  -> dict(R [n, n] fp32 block-diagonal: the R_t with the largest l1, the earliest of equals;
    blocks; iters_run: that t; l1: [l1_0, l1_1, ...] of every pass; qerr_before: qerr of R_0; qerr_after: of the returned R)."""
    codes, _, n, s = _check_itq(codes, None, blocks)
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"iters must be an int >= 0, got {iters!r}")
    if not (isinstance(tol, (int, float)) and tol >= 0):
        raise ValueError(f"tol must be a number >= 0, got {tol!r}")
    _dev_guard(codes)
    R = torch.eye(s, dtype=torch.float32).repeat(blocks, 1)
    l1s, best, before = [], None, None
    for t in range(iters + 1):
        Rd = R.to(codes.device).contiguous()
        M, l1, qerr = _itq_step(codes, Rd, n, s, 0)              # the codes were checked above, once
        l1s.append(l1)
        before = qerr if t == 0 else before
        if best is None or l1 > best[0]:
            best = (l1, Rd, t, qerr)
        if t == iters or (t >= 1 and l1 - l1s[-2] <= tol * l1s[-2]):
            break
        R = procrustes_update(M, blocks).to(torch.float32)
    return dict(R=full_rotation(best[1], blocks), blocks=blocks, iters_run=best[2], l1=l1s, qerr_before=before, qerr_after=best[3])


# ---------------------------------------------------------------------------------------------------------------
# reduction: PCA (and PCA-ITQ) of the real-valued codes to any code length ("reduction"; csrc/pca.hip)
# ---------------------------------------------------------------------------------------------------------------
REDUCE_METHODS = ("pca-itq", "pca")


def compact_projection(A: torch.Tensor, blocks: int) -> torch.Tensor:
    """[n, bits] block-structured (rows b s .. of block b are zero outside columns b t ..) -> [n, t], t = bits / blocks: row b s + l
    holds A_b[l, :] (the form the kernel takes).  An entry outside the blocks that is not zero is a ValueError."""
    n, bits = A.shape
    s = check_blocks(n, blocks)
    if bits % blocks or not blocks <= bits <= n:
        raise ValueError(f"a projection of {n} dimensions in {blocks} blocks has blocks .. n columns, a multiple of blocks; got {bits}")
    t = bits // blocks
    diag = torch.arange(blocks, device=A.device)
    out = A.reshape(blocks, s, blocks, t)[diag, :, diag, :].reshape(n, t).contiguous()
    if not torch.equal(full_projection(out, blocks), A):
        raise ValueError(f"A is not block-structured under blocks = {blocks}: an entry outside the blocks is not zero")
    return out


def full_projection(Ac: torch.Tensor, blocks: int) -> torch.Tensor:
    """[n, t] compact -> [n, blocks t] block-structured"""
    n, t = Ac.shape
    return torch.block_diag(*Ac.reshape(blocks, n // blocks, t).unbind(0)).contiguous()


def _check_pca(codes, blocks, shift=None, who="shift"):
    """The argument checks the reduction's functions share, all in front of the first launch -> (codes, shift, n, s)"""
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.float32:
        raise TypeError(f"codes must be a float32 tensor, got {getattr(codes, 'dtype', type(codes))}")
    if codes.dim() != 2:
        raise ValueError(f"codes must be 2-D [rows, n] real-valued codes, got {tuple(codes.shape)}")
    n = codes.shape[1]
    if not 1 <= n <= ITQ_MAX_DIM:
        raise ValueError(f"codes have {n} dimensions; a reduction takes 1 .. {ITQ_MAX_DIM}")
    s = check_blocks(n, blocks)
    if shift is not None:
        if not isinstance(shift, torch.Tensor) or shift.dtype != torch.float32 or tuple(shift.shape) != (n,):
            raise ValueError(f"{who} must be a float32 tensor [{n}], got {getattr(shift, 'dtype', type(shift))} "
                             f"{tuple(getattr(shift, 'shape', ()))}")
        if shift.device != codes.device:
            raise ValueError(f"{who} and the codes must be on the same device")
        if not bool(torch.isfinite(shift).all()):
            raise ValueError(f"{who} holds NaN or infinite entries")
        shift = shift.contiguous()
    if codes.numel() and not bool(torch.isfinite(codes).all()):
        raise ValueError("codes hold NaN or infinite entries: a reduction is fitted on, and applied to, finite codes")
    return codes.contiguous(), shift, n, s


def pca_moments(codes: torch.Tensor, blocks: int, shift: Optional[torch.Tensor] = None, seg_rows: Optional[int] = None, stream=None):
    """The first and second moments of y = fl32(codes - shift) (y = codes without a shift) -> (sum [n] float64, gram [n, s] float64:
    gram[b s + a, c] = sum_i y[i, b s + a] y[i, b s + c], s = n / blocks).  Inside a segment of seg_rows rows (1 .. 4096; None: chosen
    by the library) every entry is accumulated in fp32 -- a gram entry as one fmaf chain in row order --, the segments in fp64 in
    segment order: no atomics, the same bits on every call, gram exactly symmetric inside a block.  No rows: zeros."""
    codes, shift, n, s = _check_pca(codes, blocks, shift)
    seg = 0 if seg_rows is None else int(seg_rows)
    if not 0 <= seg <= ITQ_MAX_SEG or (seg_rows is not None and seg < 1):
        raise ValueError(f"seg_rows must be in [1, {ITQ_MAX_SEG}], got {seg_rows!r}")
    return _pca_moments(codes, n, s, shift, seg, True, stream)


def _pca_moments(codes, n: int, s: int, shift, seg: int, with_gram: bool, stream=None):
    """`pca_moments` behind its argument checks; with_gram=False: (sum, None)"""
    guard = _dev_guard(codes)
    lib = _lib.load()
    rows = codes.shape[0]
    total = torch.zeros(n, dtype=torch.float64, device=codes.device)
    gram = torch.zeros(n, s, dtype=torch.float64, device=codes.device) if with_gram else None
    if rows == 0:
        return total, gram
    wsb = int(lib.ch_pca_moments_workspace(rows, n, s, seg, int(with_gram)))
    ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device=codes.device)
    with guard:
        _lib.check(lib.ch_pca_moments(_lib.ptr(codes), rows, n, s, _lib.ptr(shift) if shift is not None else None, seg, _lib.ptr(total),
                                      _lib.ptr(gram) if with_gram else None, _lib.ptr(ws), ws.numel() * 8, _lib.stream_ptr(stream)),
                   "ch_pca_moments")
    return total, gram


def pca_components(cov_blocks: torch.Tensor, t: int):
    """cov_blocks [blocks, s, s] float64, symmetric -> (P [blocks, s, t] float64: per block the eigenvectors of the t largest
    eigenvalues as columns, eigenvalues [blocks, s] float64, descending).  Each component is signed so that its entry of largest
    magnitude is positive (the lowest index among equals).  A pure host function: `torch.linalg.eigh` in fp64 on the CPU."""
    if not isinstance(cov_blocks, torch.Tensor) or cov_blocks.dtype != torch.float64:
        raise TypeError(f"cov_blocks must be a float64 tensor, got {getattr(cov_blocks, 'dtype', type(cov_blocks))}")
    if cov_blocks.dim() != 3 or cov_blocks.shape[1] != cov_blocks.shape[2] or cov_blocks.shape[1] < 1:
        raise ValueError(f"cov_blocks must be [blocks, s, s], got {tuple(cov_blocks.shape)}")
    s = cov_blocks.shape[1]
    if isinstance(t, bool) or not isinstance(t, int) or not 1 <= t <= s:
        raise ValueError(f"t must be an int in [1, {s}], got {t!r}")
    C = cov_blocks.detach().to("cpu")
    if not bool(torch.isfinite(C).all()):
        raise ValueError("cov_blocks hold NaN or infinite entries")
    lam, vec = torch.linalg.eigh(C)                                  # ascending
    lam, vec = lam.flip(-1), vec.flip(-1)
    P = vec[:, :, :t].contiguous()
    lead = P.abs().argmax(dim=1, keepdim=True)                       # the first of equals
    sign = torch.where(P.gather(1, lead) < 0, -1.0, 1.0).to(torch.float64)
    return P * sign, lam.contiguous()


def project_codes(codes: torch.Tensor, mean: Optional[torch.Tensor], A: torch.Tensor, blocks: int, compact: bool = False,
                  stream=None) -> torch.Tensor:
    """[rows, n] fp32 -> [rows, bits] fp32: out[i, b t + j] = the chain acc = 0; for l = 0 .. s-1: acc = fmaf(fl32(codes[i, b s + l] -
    mean[b s + l]), A_b[l, j], acc) (mean=None: no subtraction).  A: [n, bits] block-structured as `fit_reduction` returns it, or with
    compact=True [n, t] (`compact_projection`).  A row projects to the same bits alone or in a batch; with t = s and no mean it is
    `rotate_codes`."""
    codes, mean, n, s = _check_pca(codes, blocks, mean, "mean")
    if not isinstance(A, torch.Tensor) or A.dtype != torch.float32 or A.dim() != 2 or A.shape[0] != n:
        raise ValueError(f"A must be a float32 tensor with {n} rows, got {getattr(A, 'dtype', type(A))} {tuple(getattr(A, 'shape', ()))}")
    if A.device != codes.device:
        raise ValueError("A and the codes must be on the same device")
    if not bool(torch.isfinite(A).all()):
        raise ValueError("A holds NaN or infinite entries")
    Ac = A.contiguous() if compact else compact_projection(A, blocks)
    if not 1 <= Ac.shape[1] <= s:
        raise ValueError(f"a block of {s} dimensions projects to 1 .. {s} columns, got {Ac.shape[1]}")
    return _project_codes(codes, mean, Ac, n, s, stream)


def _project_codes(codes, mean, Ac, n: int, s: int, stream=None):
    """`project_codes` behind its argument checks; Ac compact [n, t]"""
    guard = _dev_guard(codes)
    lib = _lib.load()
    t = Ac.shape[1]
    out = torch.empty(codes.shape[0], n // s * t, dtype=torch.float32, device=codes.device)
    if codes.shape[0]:
        with guard:
            _lib.check(lib.ch_pca_project(_lib.ptr(codes), codes.shape[0], n, s, _lib.ptr(mean) if mean is not None else None, _lib.ptr(Ac),
                                          t, _lib.ptr(out), _lib.stream_ptr(stream)), "ch_pca_project")
    return out


def check_reduction(n: int, bits, blocks, method="pca-itq") -> int:
    """(`bits`, `blocks`, `method`) of a reduction of n-dimensional codes (ValueError otherwise) -> t = bits / blocks"""
    check_blocks(n, blocks)
    if isinstance(bits, bool) or not isinstance(bits, int) or not blocks <= bits <= n or bits % blocks:
        raise ValueError(f"bits must be an int in [blocks, n] = [{blocks}, {n}] and a multiple of blocks = {blocks}, got {bits!r}")
    if method not in REDUCE_METHODS:
        raise ValueError(f"method must be one of {REDUCE_METHODS}, got {method!r}")
    return bits // blocks


def fit_reduction(codes: torch.Tensor, bits: int, blocks: int, iters: int = 50, method: str = "pca-itq") -> dict:
    """Fit a reduction of `codes` [N, n] fp32 to `bits` dimensions, block by block (s = n / blocks in, t = bits / blocks out):
      1. mu = fp32(sum / N) from `pca_moments` without a shift;  2. the moments of y = fl32(x - mu), C_b = (gram_b - sum_b sum_b^T / N) /
      (N - 1) in fp64;  3. P = `pca_components(C, t)`;  4. V = `project_codes(codes, mu, P)`;  5. method "pca-itq": R =
      `fit_rotation(V, blocks, iters)` and A_b = fp32(P_b R_b), the product in fp64; "pca": A = fp32(P).
    The reduced codes of a row, database or query, are `project_codes(row, mean, A, blocks)`: ONE chain, not project-then-rotate.
    -> dict(mean [n] fp32, A [n, bits] fp32 block-structured, blocks, bits, method, iters_run, explained_share: the kept eigenvalues'
    share of tr(C) (0.0 where tr(C) = 0), eigenvalues [blocks, s] (descending; a zero is a direction without variance), qerr_pca /
    qerr_after: `itq_step`'s qerr at R = I on V / on the final codes).  ValueError: bits outside [blocks, n] or no multiple of blocks,
    fewer than 2 rows, codes that are not finite."""
    codes, _, n, s = _check_pca(codes, blocks)
    t = check_reduction(n, bits, blocks, method)
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"iters must be an int >= 0, got {iters!r}")
    N = codes.shape[0]
    if N < 2:
        raise ValueError(f"a reduction is fitted on at least 2 rows (the covariance divides by N - 1), got {N}")
    _dev_guard(codes)
    dev = codes.device
    total, _ = _pca_moments(codes, n, s, None, 0, False)
    mean = (total / N).to(torch.float32)
    total, gram = _pca_moments(codes, n, s, mean, 0, True)
    sb = total.cpu().reshape(blocks, s)
    C = (gram.cpu().reshape(blocks, s, s) - sb[:, :, None] * sb[:, None, :] / N) / (N - 1)
    P, lam = pca_components(C, t)
    trace = float(C.diagonal(dim1=1, dim2=2).sum())
    share = float(lam[:, :t].sum()) / trace if trace > 0 else 0.0
    Pc = P.reshape(n, t).to(torch.float32).to(dev).contiguous()
    V = _project_codes(codes, mean, Pc, n, s)
    eye = torch.eye(t, dtype=torch.float32, device=dev).repeat(blocks, 1)
    if method == "pca-itq":
        fit = fit_rotation(V, blocks, iters)
        R = compact_rotation(fit["R"], blocks).cpu().to(torch.float64).reshape(blocks, t, t)
        Ac = (P @ R).reshape(n, t).to(torch.float32).to(dev).contiguous()
        iters_run, qerr_pca = fit["iters_run"], fit["qerr_before"]
        _, _, qerr_after = _itq_step(_project_codes(codes, mean, Ac, n, s), eye, bits, t, 0)
    else:
        Ac, iters_run = Pc, 0
        _, _, qerr_pca = _itq_step(V, eye, bits, t, 0)
        qerr_after = qerr_pca
    return dict(mean=mean, A=full_projection(Ac, blocks), blocks=blocks, bits=bits, method=method, iters_run=iters_run,
                explained_share=share, eigenvalues=lam.tolist(), qerr_pca=qerr_pca, qerr_after=qerr_after)
