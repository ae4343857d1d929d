"""Search a trained run: a `GalleryIndex` holds the packed database codes of one checkpoint and what is needed to name a hit (labels,
file paths), and ranks the database for query codes -- by the whole code, by the sub-codes of chosen concepts, by the bits a query
is sure of, or by both (`retrieval.hamming_topk_masked`), with the per-concept breakdown of every hit (`retrieval.subcode_dist`).

The code is concept-major (models/arch/coop.py, csrc/head.hip): concept c owns bits [c nbit/ncontext, (c+1) nbit/ncontext).
"""
from __future__ import annotations

import hashlib
import os
from typing import List, Optional, Sequence

import torch

from . import retrieval as rt

FORMAT = 1
RANKS = ("hamming", "asymmetric", "ternary") + rt.DENSE_METRICS
TOPK_MAX = 128    # the deepest list of the top-k scan (csrc/hamming_topk.hip); deeper ones: retrieval.hamming_ranked


class StaleIndexError(RuntimeError):
    """The index file was not encoded with this model: rebuild it."""


def checkpoint_fingerprint(path: str) -> dict:
    """{"file", "size", "sha256"} of a checkpoint file (`models/<best|last>.pth`)."""
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return {"file": os.path.basename(path), "size": os.path.getsize(path), "sha256": h.hexdigest()}


class GalleryIndex:
    """codes [G, W] int64 (packed, `retrieval.pack_sign`); nbit, ncontext; labels: None, [G] int64 class ids or [G, C] uint8 indicator
    rows; paths: None (synthetic datasets) or G paths relative to data_root; mean: None or the database mean [nbit] fp32 that was
    subtracted before packing (`zero_mean_eval`) and is subtracted from every query; transform: {"resize", "crop", "norm"} of the
    evaluation chain the database went through; fingerprint: `checkpoint_fingerprint` of the checkpoint that encoded it.
    mask: None, or the plane [G, W] int64 of the bits every database row is sure of, `retrieval.confidence_mask(codes, margin)` of the
    real codes that were packed, with `margin` the number it was built with -- what rank="ternary" needs; an index
    without it serves every other ranking as before.
    real: None, or the plane [G, nbit] fp32 of the real-valued codes that were packed (after the mean shift, where there is one) -- what
    rank="cosine" | "euclidean" | "dot" need; optional in the same way.
    groups: None, or the plane [G] int32 (values >= 0, checked here, once) of the group every row belongs to -- its album, video or
    source -- what `search(query_group=..., group_by="groups")` filters by; optional in the same way.
    rotation: None, or the learned rotation [nbit, nbit] fp32 (`fit_rotation`; DESIGN.md section 2.0, "learned rotation"), block-diagonal
    with `rotation_blocks` blocks, that the real codes went through before they were packed: every query goes through it too.
    rotation_info: what the fit reported ({"method", "blocks", "iters_run", "qerr_before", "qerr_after"}), kept with the rotation.
    reduce_mean [nbit_in], reduce_A [nbit_in, nbit], reduce_blocks, reduce_info: None, or the reduction (`fit_reduction`; DESIGN.md
    section 2.0, "reduction") that took the real codes of the model's width `nbit_in` to the `nbit` dimensions the index holds: its
    centre, its block-structured fp32 matrix, its number of blocks and what the fit reported.  Every query arrives `nbit_in` wide and
    goes through `retrieval.project_codes(q, reduce_mean, reduce_A, reduce_blocks)`, the chain the database went through; `mean` is
    then [nbit_in] too.  Without a reduction nbit_in == nbit."""

    def __init__(self, codes: torch.Tensor, nbit: int, ncontext: int, labels: Optional[torch.Tensor] = None,
                 paths: Optional[Sequence[str]] = None, data_root: Optional[str] = None, mean: Optional[torch.Tensor] = None,
                 transform: Optional[dict] = None, fingerprint: Optional[dict] = None, mask: Optional[torch.Tensor] = None,
                 margin: Optional[float] = None, real: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None,
                 rotation: Optional[torch.Tensor] = None, rotation_blocks: Optional[int] = None, rotation_info: Optional[dict] = None,
                 reduce_mean: Optional[torch.Tensor] = None, reduce_A: Optional[torch.Tensor] = None, reduce_blocks: Optional[int] = None,
                 reduce_info: Optional[dict] = None):
        nbit, ncontext = int(nbit), int(ncontext)
        if codes.dtype != torch.int64 or codes.dim() != 2 or codes.shape[1] != (nbit + 63) // 64:
            raise ValueError(f"codes must be packed int64 [G, {(nbit + 63) // 64}] for nbit = {nbit}, got {codes.dtype} {tuple(codes.shape)}")
        if ncontext < 1 or nbit % ncontext:
            raise ValueError(f"nbit = {nbit} is not a multiple of ncontext = {ncontext}")
        G = codes.shape[0]
        if labels is not None and labels.shape[0] != G:
            raise ValueError(f"{labels.shape[0]} labels for {G} codes")
        if paths is not None and len(paths) != G:
            raise ValueError(f"{len(paths)} paths for {G} codes")
        if reduce_A is not None:
            if reduce_A.dtype != torch.float32 or reduce_A.dim() != 2 or reduce_A.shape[1] != nbit or reduce_A.device != codes.device:
                raise ValueError(f"reduce_A must be a float32 matrix [nbit_in, {nbit}] on the codes' device, got {reduce_A.dtype} "
                                 f"{tuple(reduce_A.shape)} on {reduce_A.device}")
            nbit_in = int(reduce_A.shape[0])
            rt.check_reduction(nbit_in, nbit, reduce_blocks, (reduce_info or {}).get("method", "pca-itq"))
            if reduce_mean is None or reduce_mean.dtype != torch.float32 or tuple(reduce_mean.shape) != (nbit_in,) or \
                    reduce_mean.device != codes.device:
                raise ValueError(f"reduce_mean must be the float32 centre [{nbit_in}] of the reduction on the codes' device")
            self._reduce_Ac = rt.compact_projection(reduce_A.contiguous(), reduce_blocks)    # the form the kernel takes, made once
            reduce_A, reduce_mean = reduce_A.contiguous(), reduce_mean.contiguous()
        elif reduce_mean is not None or reduce_blocks is not None or reduce_info is not None:
            raise ValueError("reduce_mean / reduce_blocks / reduce_info without reduce_A")
        else:
            nbit_in, self._reduce_Ac = nbit, None
        self.reduce_mean, self.reduce_A = reduce_mean, reduce_A
        self.reduce_blocks = int(reduce_blocks) if reduce_A is not None else None
        self.reduce_info = dict(reduce_info or {}) if reduce_A is not None else None
        self._nbit_in = nbit_in
        if mean is not None and tuple(mean.shape) != (nbit_in,):
            raise ValueError(f"mean must be [{nbit_in}], got {tuple(mean.shape)}")
        if mask is not None:
            if mask.dtype != torch.int64 or tuple(mask.shape) != tuple(codes.shape) or mask.device != codes.device:
                raise ValueError(f"mask must be an int64 plane {tuple(codes.shape)} on the codes' device, got {mask.dtype} {tuple(mask.shape)} "
                                 f"on {mask.device}")
            margin = rt.check_margin(margin, "the mask plane's margin")
        elif margin is not None:
            raise ValueError("a margin without a mask plane")
        if real is not None:
            if tuple(real.shape) != (G, nbit) or real.device != codes.device:
                raise ValueError(f"real must be the plane [{G}, {nbit}] of real-valued codes on the codes' device, got {tuple(real.shape)} "
                                 f"on {real.device}")
            real = rt.check_dense_codes(real, "the real plane")
        if groups is not None:
            if groups.dtype != torch.int32 or tuple(groups.shape) != (G,) or groups.device != codes.device:
                raise ValueError(f"groups must be the int32 plane [{G}] of the rows' groups on the codes' device, got {groups.dtype} "
                                 f"{tuple(groups.shape)} on {groups.device}")
            if G and int(groups.min()) < 0:
                raise ValueError(f"groups must be >= 0 (a query's -1 means no group filter), got {int(groups.min())}")
            groups = groups.contiguous()
        if rotation is not None:
            if rotation.dtype != torch.float32 or tuple(rotation.shape) != (nbit, nbit) or rotation.device != codes.device:
                raise ValueError(f"rotation must be the float32 matrix [{nbit}, {nbit}] on the codes' device, got {rotation.dtype} "
                                 f"{tuple(rotation.shape)} on {rotation.device}")
            rt.check_blocks(nbit, rotation_blocks)
            rotation = rotation.contiguous()
        elif rotation_blocks is not None or rotation_info is not None:
            raise ValueError("rotation_blocks / rotation_info without a rotation")
        self.rotation, self.rotation_blocks = rotation, (int(rotation_blocks) if rotation is not None else None)
        self.rotation_info = dict(rotation_info or {}) if rotation is not None else None
        self.real, self.groups = real, groups
        self.codes, self.nbit, self.ncontext = codes.contiguous(), nbit, ncontext
        self.mask, self.margin = (mask.contiguous() if mask is not None else None), margin
        self.labels = labels
        self.paths = [str(p) for p in paths] if paths is not None else None
        self.data_root = str(data_root) if data_root is not None else None
        self.mean = mean.to(torch.float32) if mean is not None else None
        self.transform = dict(transform or {})
        self.fingerprint = dict(fingerprint or {})

    def __len__(self):
        return self.codes.shape[0]

    @property
    def device(self):
        return self.codes.device

    @property
    def nbit_in(self) -> int:
        """the width of the codes a query arrives with: the model's; nbit unless the index holds a reduction"""
        return self._nbit_in

    def to(self, device) -> "GalleryIndex":
        mv = lambda t: t.to(device) if t is not None else None
        return GalleryIndex(mv(self.codes), self.nbit, self.ncontext, mv(self.labels), self.paths, self.data_root, mv(self.mean),
                            self.transform, self.fingerprint, mv(self.mask), self.margin, mv(self.real), mv(self.groups),
                            mv(self.rotation), self.rotation_blocks, self.rotation_info, mv(self.reduce_mean), mv(self.reduce_A),
                            self.reduce_blocks, self.reduce_info)

    # ---- file --------------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """One torch.save file of CPU tensors and plain Python values (layout: INTEGRATION.md, "Index file")."""
        cpu = lambda t: t.detach().cpu() if t is not None else None
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = f"{path}.tmp{os.getpid()}"
        d = {"format": FORMAT, "codes": cpu(self.codes), "nbit": self.nbit, "ncontext": self.ncontext, "labels": cpu(self.labels),
             "paths": self.paths, "data_root": self.data_root, "mean": cpu(self.mean), "transform": self.transform,
             "fingerprint": self.fingerprint}
        if self.mask is not None:           # an index without the plane is the file it has always been
            d.update(mask=cpu(self.mask), margin=self.margin)
        if self.real is not None:
            d.update(real=cpu(self.real))
        if self.groups is not None:
            d.update(groups=cpu(self.groups))
        if self.rotation is not None:
            d.update(rotation=cpu(self.rotation), rotation_blocks=self.rotation_blocks, rotation_info=self.rotation_info)
        if self.reduce_A is not None:
            d.update(reduce_mean=cpu(self.reduce_mean), reduce_A=cpu(self.reduce_A), reduce_blocks=self.reduce_blocks,
                     reduce_info=self.reduce_info)
        torch.save(d, tmp)
        os.replace(tmp, path)

    def check(self, fingerprint: Optional[dict] = None, nbit: Optional[int] = None, source: str = "the index") -> None:
        """Raises StaleIndexError unless the index was encoded with the checkpoint `fingerprint` and holds codes of a model of `nbit`
        bits (`nbit_in`: a reduced index holds fewer)."""
        if nbit is not None and int(nbit) != self.nbit_in:
            raise StaleIndexError(f"{source} holds {self.nbit_in}-bit codes but the model produces {int(nbit)}-bit codes: rebuild the index "
                                  f"(rebuild_index=true)")
        if fingerprint is not None:
            mine = {k: self.fingerprint.get(k) for k in ("size", "sha256")}
            theirs = {k: fingerprint.get(k) for k in ("size", "sha256")}
            if mine != theirs:
                raise StaleIndexError(f"{source} was encoded with another checkpoint (fingerprint {mine} != {theirs}): rebuild the index "
                                      f"(rebuild_index=true)")

    @classmethod
    def load(cls, path: str, fingerprint: Optional[dict] = None, nbit: Optional[int] = None) -> "GalleryIndex":
        """The index of `save`, on the CPU; with `fingerprint` / `nbit` given, `check`ed against them."""
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise StaleIndexError(f"{path} is not a gallery index of format {FORMAT}: rebuild the index (rebuild_index=true)")
        index = cls(d["codes"], d["nbit"], d["ncontext"], d["labels"], d["paths"], d["data_root"], d["mean"], d["transform"],
                    d["fingerprint"], d.get("mask"), d.get("margin"), d.get("real"), d.get("groups"), d.get("rotation"),
                    d.get("rotation_blocks"), d.get("rotation_info"), d.get("reduce_mean"), d.get("reduce_A"), d.get("reduce_blocks"),
                    d.get("reduce_info"))
        index.check(fingerprint, nbit, source=path)
        return index

    # ---- learned rotation --------------------------------------------------------------------------------------------------------
    @property
    def keeps_concepts(self) -> bool:
        """whether `concepts=`, concept_dist and the per-concept evaluation still mean the concepts: no rotation, or one whose blocks
        lie inside the sub-codes"""
        return (self.rotation is None or self.rotation_blocks % self.ncontext == 0) and \
            (self.reduce_A is None or self.reduce_blocks % self.ncontext == 0)

    def fit_rotation(self, blocks: Optional[int] = None, iters: int = 50) -> "GalleryIndex":
        """The index under a rotation fitted to its real plane (`retrieval.fit_rotation`; blocks=None: one block per concept): its real
        plane holds the rotated codes, its packed codes their signs, its mask plane -- where the index has one -- is rebuilt from them
        under the same margin, and every query is rotated in `search`.  An index without the real plane, or one that is rotated
        already, raises ValueError."""
        if self.real is None:
            raise ValueError("fit_rotation needs the index's real plane, which this index was built without: rebuild it "
                             "(exp=search rotate=itq rebuilds it by itself; rebuild_index=true forces it)")
        if self.rotation is not None:
            raise ValueError("this index is rotated already: fit a rotation on the index as it was built")
        blocks = self.ncontext if blocks is None else blocks
        rt.check_blocks(self.nbit, blocks)
        fit = rt.fit_rotation(self.real, blocks, iters)
        real = rt.rotate_codes(self.real, fit["R"], blocks)
        info = dict(method="itq", blocks=blocks, iters_run=fit["iters_run"], qerr_before=fit["qerr_before"], qerr_after=fit["qerr_after"])
        return GalleryIndex(rt.pack_sign(real), self.nbit, self.ncontext, self.labels, self.paths, self.data_root, self.mean, self.transform,
                            self.fingerprint, rt.confidence_mask(real, self.margin) if self.mask is not None else None, self.margin, real,
                            self.groups, fit["R"], blocks, info, self.reduce_mean, self.reduce_A, self.reduce_blocks, self.reduce_info)

    # ---- reduction ---------------------------------------------------------------------------------------------------------------
    def fit_reduction(self, bits: int, blocks: Optional[int] = None, iters: int = 50, method: str = "pca-itq") -> "GalleryIndex":
        """A NEW index of `bits`-bit codes under a reduction fitted to this index's real plane (`retrieval.fit_reduction`; blocks=None:
        one block per concept): nbit = bits, its real plane holds the reduced codes, its packed codes their signs, its mask plane --
        where the index has one -- is rebuilt from them under the same margin, and every query (nbit_in wide) is reduced in `search`.
        With blocks a multiple of ncontext, `concepts=[...]` addresses sub-codes of bits / ncontext bits.  An index without the real
        plane, one that is rotated already or one that is reduced already raises ValueError."""
        if self.real is None:
            raise ValueError("fit_reduction needs the index's real plane, which this index was built without: rebuild it "
                             "(exp=search reduce=pca-itq rebuilds it by itself; rebuild_index=true forces it)")
        if self.rotation is not None:
            raise ValueError("this index is rotated already: fit a reduction on the index as it was built")
        if self.reduce_A is not None:
            raise ValueError("this index is reduced already: fit a reduction on the index as it was built")
        blocks = self.ncontext if blocks is None else blocks
        rt.check_reduction(self.nbit, bits, blocks, method)
        if bits % self.ncontext:
            raise ValueError(f"bits = {bits} is not a multiple of ncontext = {self.ncontext}: the reduced code keeps ncontext sub-codes")
        fit = rt.fit_reduction(self.real, bits, blocks, iters, method)
        real = rt.project_codes(self.real, fit["mean"], fit["A"], blocks)
        info = {k: fit[k] for k in ("method", "bits", "blocks", "iters_run", "explained_share", "qerr_pca", "qerr_after")}
        info["bits_in"] = self.nbit
        return GalleryIndex(rt.pack_sign(real), bits, self.ncontext, self.labels, self.paths, self.data_root, self.mean, self.transform,
                            self.fingerprint, rt.confidence_mask(real, self.margin) if self.mask is not None else None, self.margin, real,
                            self.groups, None, None, None, fit["mean"], fit["A"], blocks, info)

    # ---- search ------------------------------------------------------------------------------------------------------------------
    def resolve(self, rel: Optional[str]) -> Optional[str]:
        """A hit's path as a file name: a relative path is looked up as the list-file datasets look it up (as it stands, under
        data_root, under the directory two levels above data_root) and taken under data_root when no such file exists."""
        if rel is None:
            return None
        if os.path.isabs(rel) or self.data_root is None:
            return rel
        for cand in (rel, os.path.join(self.data_root, rel), os.path.join(os.path.dirname(os.path.dirname(self.data_root)), rel)):
            if os.path.exists(cand):
                return cand
        return os.path.join(self.data_root, rel)

    def search(self, query_codes: torch.Tensor, k: int, concepts: Optional[Sequence[int]] = None, margin: float = 0.0,
               rank: str = "hamming", weight_bits: int = 8, radius: Optional[int] = None, mean_shift: bool = True,
               shortlist: Optional[int] = None, rows: Optional[torch.Tensor] = None, labels_in: Optional[Sequence[int]] = None,
               labels_out: Optional[Sequence[int]] = None, query_group: Optional[torch.Tensor] = None, group_mode: str = "only",
               group_by: str = "groups") -> dict:
        """query_codes: [Qn, nbit] fp32 as the model returns them (the database mean, if the index holds one, is subtracted here;
        mean_shift=False leaves them as they are -- text queries, whose codes are centre-side and never shifted: DESIGN.md section 2.0;
        a rotated index then rotates them, shifted or not, before anything else reads them; a reduced index takes them [Qn, nbit_in]
        wide and reduces them first, in the same place).
        Ranks the database by ascending (distance, index) and returns
          idx [Qn, k] int64 (-1 past the end of the database), dist [Qn, k] int32: the ranking distance, popcount((q ^ g) & mask);
          concept_dist [Qn, k, ncontext] int32: the UNMASKED distance inside every concept's sub-code (they sum to the whole-code
            distance whatever the mask, so for a hit ranked by concepts 0 and 2 they still say how far the other concepts are);
          bits [Qn] int64: the number of unmasked bits of each query;
          labels: None or the hits' labels [Qn, k(, C)] (class id -1 / zero rows where idx is -1); paths: None or Qn lists of k paths.
        concepts: rank by these concepts' sub-codes only (one mask shared by all queries).  margin > 0: every query ignores its own
        bits with |code| <= margin.  Both: the per-query mask is the AND of the two.  Neither: the unmasked scan.
        rank: "hamming" (above) or "asymmetric": the same mask, but a disagreement on bit j costs the query's own |code_j|, quantised to
        weight_bits (4 or 8) bits against the largest unmasked |code| of that query (`retrieval.weight_planes`).
        dist is then that weighted distance, and the dict also holds rank, weight_bits and dist_max [Qn] int32, the sum of a query's
        weights (the distance of a row that disagrees on every unmasked bit); everything else is as under "hamming".
        k > 128: the list comes from `retrieval.hamming_ranked` (any depth); built for rank="hamming" without a margin (the whole code
        or `concepts`); the other combinations raise ValueError.
        radius: hash lookup -- only rows whose ranking distance (the masked one under `concepts` / `margin`) is <= radius stay; idx and
        dist are -1 behind them, as past the end of the database.  Not defined for rank="asymmetric" (ValueError).
        rank="ternary": both sides are ternary codes -- the database rows under the index's own margin (its mask plane; an index without
        one raises ValueError), the queries under `margin` -- and dist is K = nbit - t_q . t_g in HALF bits (a bit either side is unsure of
        costs 1, a disagreement both are sure of 2); dist_bits = K / 2.  `concepts` clears the query's mask outside the chosen sub-codes and
        nbit becomes the number of bits in play, so K stays the distance on those bits; radius keeps K <= 2 radius; bits counts the
        query's sure bits in play and dist_max = bits in play + bits; k <= 128.  The dict also holds rank and index_margin.
        rank="cosine" | "euclidean" | "dot": the ranking of the real-valued codes themselves (`retrieval.dense_topk`; DESIGN.md section
        2.0) against the index's real plane (an index without one raises ValueError); dist is fp32 -- 1 - cos, the squared Euclidean
        distance or the negated dot product -- and +inf where idx is -1.  No `concepts`, no margin, no radius (ValueError), k <= 128;
        concept_dist and bits describe the sign codes of the hits as under "hamming".
        shortlist = m under a dense rank: the two-stage list (`retrieval.rerank_topk`; DESIGN.md section 2.0, "two-stage") -- the first m
        rows by ascending (Hamming distance, index) of the sign codes, ordered by the dense distance and cut at k.  1 <= k <= m <= 4096,
        so k may exceed 128; `radius` is then allowed and restricts the shortlist to rows within that many bits.  The dict also holds
        shortlist.  Under any other rank a shortlist is a ValueError.
        Filtered search ("filtered search"): which rows may be hits at all, decided inside the scan, so a list
        is as full as the admitted rows allow (idx = dist = -1 behind them).
          rows: bool [G], or the packed bitmap of `retrieval.row_bitmap`: the rows that may be hits (e.g. not deleted).
          labels_in / labels_out: class ids; the row's class is in the set / is not in it (single-label index), the row has any of the
            classes / none of them (indicator rows).  They need the index's labels and combine with `rows` by AND into ONE bitmap for
            all queries (torch ops on the index's device).
          query_group: int64 [Qn], one group per query (-1: no group filter for that query), with group_mode "only" (hits of that group
            alone) or "exclude" (of every other group) and group_by = where a row's group comes from: "groups" (the index's groups
            plane), "labels" (the row's class id; single-label indexes) or "row" (the row's own index: query_group = the query's own
            database row with group_mode="exclude" is "neighbours of a database image without the image itself").
        They compose with `concepts`, `margin`, `radius` (cut after the filter) and rank "hamming" | "asymmetric" | "ternary" at
        k <= 128: those lists come from the one top-k scan (`retrieval.hamming_topk_filtered`, `ternary_topk_filtered`).  Lists deeper
        than 128, the dense ranks and a shortlist do not go through that scan, and a filter under them raises ValueError.
        Under a filter the dict also holds rows_admitted: the number of rows the shared bitmap admits (G where there is none), so a
        short list explains itself."""
        if rank not in RANKS:
            raise ValueError(f"rank must be one of {RANKS}, got {rank!r}")
        if concepts is not None and self.reduce_A is not None and self.reduce_blocks % self.ncontext:
            raise ValueError(f"concepts with a reduction of {self.reduce_blocks} blocks is not built: a block would straddle the sub-codes "
                             f"of the {self.ncontext} concepts (fit it with blocks a multiple of {self.ncontext})")
        if concepts is not None and not self.keeps_concepts:
            raise ValueError(f"concepts with a rotation of {self.rotation_blocks} blocks is not built: a block would straddle the sub-codes "
                             f"of the {self.ncontext} concepts (fit it with blocks a multiple of {self.ncontext})")
        if shortlist is not None and rank not in rt.DENSE_METRICS:
            raise ValueError(f"shortlist with rank='{rank}' is not built: a shortlist is reranked by a dense rank, one of {rt.DENSE_METRICS}")
        filtered = any(v is not None for v in (rows, labels_in, labels_out, query_group))
        if filtered:
            names = ", ".join(n for n, v in (("rows", rows), ("labels_in", labels_in), ("labels_out", labels_out), ("query_group", query_group))
                              if v is not None)
            why = f"the filter is a predicate of the top-k scan (k <= {TOPK_MAX}, rank 'hamming', 'asymmetric' or 'ternary')"
            if shortlist is not None:
                raise ValueError(f"a filter ({names}) with a shortlist is not built: {why}, and a two-stage list does not go through it")
            if rank in rt.DENSE_METRICS:
                raise ValueError(f"a filter ({names}) with rank='{rank}' is not built: {why}, and the dense ranks do not go through it")
            if int(k) > TOPK_MAX:
                raise ValueError(f"a filter ({names}) with k = {int(k)} > {TOPK_MAX} is not built: {why}, and deeper lists do not go through it")
        if rank in rt.DENSE_METRICS:
            return self._search_dense(query_codes, int(k), concepts, margin, rank, radius, mean_shift, shortlist)
        if rank == "asymmetric" and int(weight_bits) not in rt.WEIGHT_BITS:
            raise ValueError(f"weight_bits must be one of {rt.WEIGHT_BITS}, got {weight_bits!r}")
        k = int(k)
        deep = k > TOPK_MAX
        if radius is not None:
            if rank == "asymmetric":
                raise ValueError("radius with rank='asymmetric' is not built: a radius is a number of bits, the asymmetric distance is not")
            radius = int(radius)
            if not 0 <= radius <= 64 * self.codes.shape[1]:
                raise ValueError(f"radius must be in [0, {64 * self.codes.shape[1]}], got {radius}")
        if rank == "ternary" and self.mask is None:
            raise ValueError("rank='ternary' needs the index's mask plane, which this index was built without: build it with index_margin=<m> "
                             "(exp=search rank=ternary index_margin=<m> rebuild_index=true)")
        if rank == "ternary":
            margin = rt.check_margin(margin, "rank='ternary': the query margin")
        if deep and rank != "hamming":
            raise ValueError(f"k = {k} > {TOPK_MAX} with rank='{rank}' is not built: lists deeper than {TOPK_MAX} rank by the Hamming distance")
        if deep and margin > 0:
            raise ValueError(f"k = {k} > {TOPK_MAX} with margin > 0 is not built: lists deeper than {TOPK_MAX} take one mask shared by all "
                             f"queries (concepts), not a mask per query")
        dev = self.device
        codes, q, flt = self._query(query_codes, mean_shift, refuse=None if not filtered else
                                    lambda Qn: self._filter(Qn, rows, labels_in, labels_out, query_group, group_mode, group_by))
        Qn = codes.shape[0]
        keep = torch.ones(self.nbit, dtype=torch.bool, device=dev)
        mask = None
        if concepts is not None:
            shared = rt.concept_mask(self.nbit, self.ncontext, concepts)
            sb = self.nbit // self.ncontext
            keep = torch.zeros(self.nbit, dtype=torch.bool, device=dev)
            for c in concepts:
                keep[int(c) * sb:(int(c) + 1) * sb] = True
            mask = shared.to(dev)
        keep = keep[None, :].expand(Qn, self.nbit)
        if rank == "ternary":
            q3 = rt.pack_ternary(codes, margin)
            keep = keep & (codes.abs() > margin)
            nbit_play = self.nbit
            if mask is not None:            # the chosen concepts: the query is unsure of every other bit, and only theirs are in play
                q3 = q3 & mask[None, None, :]
                nbit_play = len(concepts) * (self.nbit // self.ncontext)
        elif margin > 0:
            conf = rt.confidence_mask(codes, float(margin))
            mask = conf if mask is None else conf & mask[None, :]
            keep = keep & (codes.abs() > float(margin))
        extra = {}
        if rank == "asymmetric":
            planes, wsum = rt.weight_planes(codes, int(weight_bits), mask)
            idx, dist = self._asymmetric_list(q, planes, k, flt)
            extra = dict(rank=rank, weight_bits=int(weight_bits), dist_max=wsum)
        elif rank == "ternary":
            g3 = torch.stack([self.codes & self.mask, self.mask], dim=1)
            if nbit_play == 0:
                raise ValueError("rank='ternary' with an empty set of concepts leaves no bit in play")
            idx, dist = self._ternary_list(q3, g3, nbit_play, k, flt)
            if radius is not None:
                far = dist > 2 * radius
                idx, dist = idx.masked_fill(far, -1), dist.masked_fill(far, -1)
            bits_sure = keep.sum(1)
            extra = dict(rank=rank, index_margin=self.margin, dist_bits=torch.where(dist < 0, -torch.ones_like(dist, dtype=torch.float64), dist.double() / 2),
                         dist_max=(bits_sure + nbit_play).to(torch.int32))
        elif deep:
            idx, dist = rt.hamming_ranked(q, self.codes, k, radius=radius, mask=mask)
        else:
            idx, dist = self._hamming_list(q, mask, k, flt)
        if flt is not None:              # an unfiltered search returns the keys it always has
            extra["rows_admitted"] = len(self) if flt["allow"] is None else rt.bitmap_count(flt["allow"], len(self))
        if radius is not None and not deep and rank != "ternary":
            far = dist > radius
            idx, dist = idx.masked_fill(far, -1), dist.masked_fill(far, -1)
        out = dict(idx=idx, dist=dist, concept_dist=rt.subcode_dist(q, self.codes, idx, self.nbit, self.ncontext),
                   bits=keep.sum(1), labels=None, paths=None, **extra)
        return self._name_hits(out)

    def _query(self, query_codes: torch.Tensor, mean_shift: bool, dense: bool = False, refuse=None):
        """The prologue of a search: the checked query codes on the index's device as fp32 (dense: finite too, checked before
        anything is launched), minus the database mean where there is one and mean_shift asks for it -> (codes, their packed signs,
        refuse(Qn) or None).  refuse: the caller's checks that need the number of queries (the filter); they raise behind the checks
        of the codes and in front of the first kernel."""
        if query_codes.dim() != 2 or query_codes.shape[1] != self.nbit_in:
            raise ValueError(f"query codes must be [Qn, {self.nbit_in}], got {tuple(query_codes.shape)}")
        if dense:
            query_codes = rt.check_dense_codes(query_codes, "query codes")
        codes = query_codes.to(self.device, torch.float32)
        if self.mean is not None and mean_shift:
            codes = codes - self.mean[None, :]
        checked = None if refuse is None else refuse(codes.shape[0])
        if self.reduce_A is not None:           # every query, shifted or not: the chain the database went through, its centre included
            codes = rt.project_codes(codes.contiguous(), self.reduce_mean, self._reduce_Ac, self.reduce_blocks, compact=True)
        if self.rotation is not None:
            codes = rt.rotate_codes(codes.contiguous(), self.rotation, self.rotation_blocks)
        return codes, rt.pack_sign(codes), checked

    # the list of one rank at k <= TOPK_MAX; flt: None, or the arguments of `_filter`
    def _hamming_list(self, q, mask, k: int, flt):
        if flt is not None:
            return rt.hamming_topk_filtered(q, self.codes, k, mask=mask, **flt)
        return rt.hamming_topk(q, self.codes, k) if mask is None else rt.hamming_topk_masked(q, self.codes, mask, k)

    def _asymmetric_list(self, q, planes, k: int, flt):
        if flt is not None:
            return rt.hamming_topk_filtered(q, self.codes, k, planes=planes, **flt)
        return rt.hamming_topk_weighted(q, planes, self.codes, k)

    def _ternary_list(self, q3, g3, nbit: int, k: int, flt):
        if flt is not None:
            return rt.ternary_topk_filtered(q3, g3, nbit, k, **flt)
        return rt.ternary_topk(q3, g3, nbit, k)

    def _label_rows(self, ids, what: str) -> torch.Tensor:
        """bool [G]: the rows that carry one of the classes `ids` (labels_in / labels_out)"""
        if self.labels is None:
            raise ValueError(f"{what} needs the index's labels, which this index was built without")
        ids = [int(c) for c in ids]
        if self.labels.dim() == 1:
            return torch.isin(self.labels, torch.tensor(ids, dtype=self.labels.dtype, device=self.labels.device))
        C = self.labels.shape[1]
        if any(c < 0 or c >= C for c in ids):
            raise ValueError(f"{what} = {ids} outside the index's classes [0, {C})")
        return (self.labels[:, ids] != 0).any(1)

    def _filter(self, Qn: int, rows, labels_in, labels_out, query_group, group_mode: str, group_by: str) -> dict:
        """The filter arguments of `retrieval.hamming_topk_filtered` / `ternary_topk_filtered` for one `search`: allow (ONE packed
        bitmap: rows AND labels_in AND NOT labels_out, None where none of them is given), group, want, exclude.  Every refusal comes
        before anything is launched."""
        G, dev = len(self), self.device
        words = (G + 63) // 64
        if group_mode not in ("only", "exclude"):
            raise ValueError(f"group_mode must be 'only' or 'exclude', got {group_mode!r}")
        if group_by not in ("groups", "labels", "row"):
            raise ValueError(f"group_by must be 'groups', 'labels' or 'row', got {group_by!r}")
        packed = None
        adm = None
        if rows is not None:
            if not isinstance(rows, torch.Tensor) or (rows.dtype, tuple(rows.shape)) not in ((torch.bool, (G,)), (torch.int64, (words,))):
                raise ValueError(f"rows must be a bool tensor [{G}] or a packed int64 bitmap [{words}] (retrieval.row_bitmap), got "
                                 f"{getattr(rows, 'dtype', type(rows))} {tuple(getattr(rows, 'shape', ()))}")
            rows = rows.to(dev)
            if rows.dtype == torch.bool:
                adm = rows
            else:
                packed = rows
        if labels_in is not None:
            hit = self._label_rows(labels_in, "labels_in").to(dev)
            adm = hit if adm is None else adm & hit
        if labels_out is not None:
            hit = ~self._label_rows(labels_out, "labels_out").to(dev)
            adm = hit if adm is None else adm & hit
        if adm is not None:
            packed = rt.row_bitmap(adm) if packed is None else packed & rt.row_bitmap(adm)
        group = want = None
        if query_group is not None:
            if not isinstance(query_group, torch.Tensor) or query_group.dtype != torch.int64 or tuple(query_group.shape) != (Qn,):
                raise ValueError(f"query_group must be an int64 tensor [{Qn}] (-1 = no group filter for that query), got "
                                 f"{getattr(query_group, 'dtype', type(query_group))} {tuple(getattr(query_group, 'shape', ()))}")
            want = query_group.to(dev)
            if group_by == "groups":
                if self.groups is None:
                    raise ValueError("group_by='groups' needs the index's groups plane, which this index was built without")
                group = self.groups
            elif group_by == "labels":
                if self.labels is None or self.labels.dim() != 1:
                    raise ValueError("group_by='labels' needs single-label class ids; this index holds " +
                                     ("no labels" if self.labels is None else "indicator rows (filter them with labels_in / labels_out)"))
                group = self.labels.to(dev, torch.int32)
        return dict(allow=packed, group=group, want=want, exclude=group_mode == "exclude")

    def _search_dense(self, query_codes, k: int, concepts, margin, rank: str, radius, mean_shift: bool, shortlist=None) -> dict:
        """`search` under a dense rank"""
        if concepts is not None or (radius is not None and shortlist is None) or (margin is not None and float(margin) != 0.0):
            raise ValueError(f"rank='{rank}' ranks by the whole real-valued code: concepts, a query margin and a radius are defined on bits "
                             "and are not built under it" + (" (a radius restricts a shortlist: shortlist=<m>)" if radius is not None else ""))
        if shortlist is not None:
            k, shortlist = rt.check_shortlist(k, shortlist)
            if radius is not None and not 0 <= int(radius) <= 64 * self.codes.shape[1]:
                raise ValueError(f"radius must be in [0, {64 * self.codes.shape[1]}], got {radius}")
        elif not 1 <= k <= rt.DENSE_MAX_K:
            raise ValueError(f"k = {k} with rank='{rank}' is not built: the dense scan keeps lists of 1 .. {rt.DENSE_MAX_K} "
                             f"(a two-stage list goes to {rt.RERANK_MAX}: shortlist=<m>)")
        if self.real is None:
            raise ValueError(f"rank='{rank}' needs the index's real plane, which this index was built without: rebuild it "
                             f"(exp=search rank={rank} rebuilds it by itself; rebuild_index=true forces it)")
        codes, q, _ = self._query(torch.as_tensor(query_codes), mean_shift, dense=True)
        dev = self.device
        extra = {}
        if shortlist is not None:
            idx, dist = rt.rerank_topk(codes, self.real, rank, k, shortlist, None if radius is None else int(radius), q, self.codes)
            extra = dict(shortlist=shortlist)
        else:
            idx, dist = rt.dense_topk(rt.prepare_dense(codes, rank), rt.prepare_dense(self.real, rank), rank, k)
        out = dict(idx=idx, dist=dist, concept_dist=rt.subcode_dist(q, self.codes, idx, self.nbit, self.ncontext),
                   bits=torch.full((codes.shape[0],), self.nbit, dtype=torch.int64, device=dev), labels=None, paths=None, rank=rank, **extra)
        return self._name_hits(out)

    def _name_hits(self, out: dict) -> dict:
        idx = out["idx"]
        if self.labels is not None:
            lab = self.labels[idx.clamp_min(0)]
            miss = idx < 0
            out["labels"] = lab.masked_fill(miss, -1) if lab.dim() == 2 else lab.masked_fill(miss[..., None], 0)
        if self.paths is not None:
            rows: List[List[Optional[str]]] = []
            for hits in idx.tolist():
                rows.append([self.paths[i] if i >= 0 else None for i in hits])
            out["paths"] = rows
        return out
