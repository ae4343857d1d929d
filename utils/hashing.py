"""`utils.hashing` -- retrieval metrics under the reference's import path, computed by the HIP kernels.

The reference imports `calculate_mAP`, `calculate_pr_curve` (experiments/test_hashing.py:15) and `get_hamm_dist`
(trainers/orthohash.py:17) from an un-vendored package whose source is not in the snapshot; signatures and return
arity below are those of the call sites (experiments/test_hashing.py:106-131,153-167; experiments/train_helper.py:228-241;
trainers/orthohash.py:362).  Semantics are the published definition of SURVEY.md section 8c / DESIGN.md section 2.

Inputs may be CPU or GPU float tensors (the reference hands over CPU tensors, trainers/base.py:291-296); they are moved
to the current GPU, sign-packed to uint64 and never expanded to a (Qn, G) matrix.  In a multi-rank run the trainer hands over
`concepthash_amd.distributed.RowShard`s -- each rank's rows, still on the GPU that encoded them: the database is scanned in place,
only the packed query codes are all-gathered.
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from concepthash_amd import retrieval as rt


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("utils.hashing needs a GPU (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _check(dist_metric, threshold, landmark_gt):
    if dist_metric != "hamming":
        raise NotImplementedError(f"dist_metric='{dist_metric}': only 'hamming' is built under this argument (what the reference's "
                                  "un-vendored package does with another value cannot be read); the cosine, Euclidean and dot rankings "
                                  "of the real-valued codes are asked for by name: rank=\"cosine\" | \"euclidean\" | \"dot\"")
    if threshold not in (0, 0.0):
        raise NotImplementedError("threshold != 0 is not built: what the reference's un-vendored package does with it cannot be read; "
                                  "ternary codes are ranked with rank=\"ternary\", margin=<m> (every reference call site passes 0)")
    if landmark_gt is not None:
        raise NotImplementedError("landmark ground-truth evaluation is outside the ConceptHash path")


def _labels(t: torch.Tensor, dev):
    t = torch.as_tensor(t)
    return t.to(dev)


def _sharded():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


# The tie bracket of the last calculate_mAP(..., tie_bracket=True) call: {"mAP_low", "mAP_high", "precisions_low", "precisions_high",
# "recalls_low", "recalls_high"} (the return arity of calculate_mAP is the reference's and cannot grow); None after any other call.
last_tie_bracket = None
# Hash lookup of the last calculate_mAP(..., radii=[...]) call, the same pattern: {"radii", "precisions_radius", "recalls_radius",
# "retrieved_radius", "empty_radius"} (lists, one entry per radius); None after any other call.
last_hash_lookup = None
# The tie expectation of the last calculate_mAP(..., tie_expected=True) call, the same pattern: {"mAP_expected", "precisions_expected",
# "recalls_expected"} -- the mean over every order of equal-distance rows; None after any other call.
last_tie_expected = None
# The two-stage figures of the last calculate_mAP(..., rank=<dense>, shortlist=m) call, the same pattern: {"metric", "shortlist", "R"
# (the effective R: -1 becomes the shortlist), "agreement" ({k: share of the exhaustive dense top-k found in the two-stage top-k})};
# None after any other call.
last_rerank = None


def _evaluate(db_codes, db_labels, test_codes, test_labels, R, ks, remove_first, skip=False, tie=False, radii=None, expected=False):
    dev = _device()
    look = {} if radii is None else {"radii": radii}    # the sharded evaluator refuses it (NotImplementedError)
    if expected:
        look["tie_expected"] = True
    from concepthash_amd.distributed import RowShard
    if isinstance(db_codes, RowShard) or isinstance(test_codes, RowShard):
        # multi-rank evaluation on the outputs of BaseTrainer.inference_one_epoch: every rank's block of the DATABASE stays on the
        # GPU that encoded it and is scanned there; the QUERIES' packed codes (8-16 bytes each) and compact labels are all-gathered
        from concepthash_amd.distributed import ShardedRetrieval, _all_gather_ragged
        if not (isinstance(db_codes, RowShard) and isinstance(db_labels, RowShard)):
            raise TypeError("sharded evaluation: database codes and labels must both be RowShards")
        g = rt.pack_sign(db_codes.local.to(dev, torch.float32))
        sr = ShardedRetrieval(g, db_labels.local.to(dev))
        if isinstance(test_codes, RowShard):
            q = sr.gather_queries(rt.pack_sign(test_codes.local.to(dev, torch.float32)))
        else:
            q = rt.pack_sign(torch.as_tensor(test_codes).to(dev, torch.float32))
        if isinstance(test_labels, RowShard):
            tl = test_labels.local.to(dev)
            if tl.dim() == 2:
                tl = (tl != 0).to(torch.uint8)                      # indicator rows travel as bytes
            ql, _ = _all_gather_ragged(tl.contiguous(), sr.group)
        else:
            ql = _labels(test_labels, dev)
        return sr.evaluate(q, ql, R=R, ks=ks, remove_first=remove_first, skip_queries_without_relevant=skip, tie_bracket=tie, **look)
    q = rt.pack_sign(torch.as_tensor(test_codes).to(dev, torch.float32))
    if _sharded():
        # replicated inputs under an initialised process group (a caller that gathered its codes): every rank takes its block
        import torch.distributed as dist
        from concepthash_amd.distributed import ShardedRetrieval, shard_bounds
        b = shard_bounds(db_codes.shape[0], dist.get_world_size())
        lo, hi = b[dist.get_rank()], b[dist.get_rank() + 1]
        g = rt.pack_sign(torch.as_tensor(db_codes[lo:hi]).to(dev, torch.float32))
        sr = ShardedRetrieval(g, _labels(db_labels[lo:hi], dev))
        return sr.evaluate(q, _labels(test_labels, dev), R=R, ks=ks, remove_first=remove_first, skip_queries_without_relevant=skip,
                           tie_bracket=tie, **look)
    g = rt.pack_sign(torch.as_tensor(db_codes).to(dev, torch.float32))
    return rt.evaluate(q, g, _labels(test_labels, dev), _labels(db_labels, dev), R=R, ks=ks, remove_first=remove_first,
                       skip_queries_without_relevant=skip, tie_bracket=tie, **look)


DENSE_RANKS = tuple(rt.DENSE_METRICS)      # "cosine", "euclidean", "dot": the rankings of the real-valued codes themselves
RANKS = ("hamming", "asymmetric", "ternary") + DENSE_RANKS


def _single_process(rank, *operands):
    from concepthash_amd.distributed import RowShard
    if any(isinstance(x, RowShard) for x in operands) or _sharded():
        raise NotImplementedError(f"rank='{rank}' is evaluated by one process on a whole database; the sharded form is not built "
                                  "(its bins are additive over gallery shards)")


def _evaluate_ranked(rank, db_codes, db_labels, test_codes, test_labels, R, ks, remove_first, skip, weight_bits=None, margin=None,
                     shortlist=None):
    """Every rank but "hamming": one process on a whole database; what differs is how the two code sets are prepared.
    "asymmetric": the queries keep their real values (`retrieval.evaluate_weighted`), the database is sign-packed as ever.
    "ternary": both code sets become ternary codes under one margin (`retrieval.pack_ternary`), ranked by K.
    "cosine" | "euclidean" | "dot": both code sets stay real-valued (`retrieval.evaluate_dense`)."""
    _single_process(rank, db_codes, db_labels, test_codes, test_labels)
    how = dict(R=R, ks=ks, remove_first=remove_first, skip_queries_without_relevant=skip)
    if rank in DENSE_RANKS:
        # finiteness is checked where the codes are (a host tensor never reaches the GPU with a NaN in it)
        q, g = rt.check_dense_codes(test_codes, "test_codes"), rt.check_dense_codes(db_codes, "db_codes")
        dev = _device()
        if shortlist is not None:       # the two-stage list: a Hamming shortlist of the sign codes, ordered by the dense distance
            return rt.evaluate_reranked(q.to(dev), g.to(dev), _labels(test_labels, dev), _labels(db_labels, dev), rank, shortlist, **how)
        return rt.evaluate_dense(q.to(dev), g.to(dev), _labels(test_labels, dev), _labels(db_labels, dev), rank, **how)
    dev = _device()
    db = torch.as_tensor(db_codes).to(dev, torch.float32)
    test = torch.as_tensor(test_codes).to(dev, torch.float32)
    if rank == "asymmetric":
        return rt.evaluate_weighted(test, rt.pack_sign(db), _labels(test_labels, dev), _labels(db_labels, dev), bits=int(weight_bits), **how)
    g3 = rt.pack_ternary(db, margin)
    return rt.evaluate_ternary(rt.pack_ternary(test, margin), g3, db.shape[1], _labels(test_labels, dev), _labels(db_labels, dev), **how)


def calculate_mAP(db_codes, db_labels, test_codes, test_labels, R, threshold=0., dist_metric="hamming", PRs=None,
                  remove_first_retrieved=False, landmark_gt=None, db_id=None, test_id=None, multiclass=False,
                  skip_queries_without_relevant=False, tie_bracket=False, radii=None, rank="hamming", weight_bits=8, margin=None, shortlist=None,
                  tie_expected=False):
    """-> (mAP, recalls, precisions); `mAP` is a list when `R` is a list (experiments/test_hashing.py:124-128).
    R <= 0 means the whole database.  One histogram pass + one AP pass whatever the length of R and PRs: every R and every k
    is a rank limit of the same gallery scan.
    skip_queries_without_relevant (not a reference argument; the reference's un-vendored `utils.hashing` cannot be read, so the one
    convention that changes numbers at R < database size is a switch): False (default) = a query with no relevant row inside its top
    R contributes AP = 0 to the mean; True = such queries are left out of the mean, as the HashNet /
    OrthoHash family of evaluators does.  mAP@all on CUB-200 / Cars196 / NABirds is the same under both.
    tie_bracket (not a reference argument): also compute the smallest / largest value of every statistic over all orders of the
    database rows that share a Hamming distance -- the one thing another implementation's sort may do
    differently.  The triple returned is unchanged; the bracket is left in the module attribute `last_tie_bracket` (a dict with
    mAP_low, mAP_high, precisions_low/high, recalls_low/high; lists where the triple has lists), which is None after a call without it.
    tie_expected (not a reference argument): also compute the MEAN of every statistic over those orders, every set of equal-distance
    rows uniformly permuted ("tie expectation") -- the figure that depends on no sort implementation, inside the
    bracket.  The triple is unchanged; `last_tie_expected` holds mAP_expected, precisions_expected, recalls_expected, and is None after
    a call without it.  Hamming rank only, and not together with skip_queries_without_relevant (ValueError: the set of counted queries
    would depend on the tie order).
    radii (not a reference argument): a list of Hamming radii -- also compute hash lookup within each ("P@H<=r": precision, recall, rows
    retrieved and the share of queries retrieving nothing) from the histogram the call holds anyway; left in the
    module attribute `last_hash_lookup` in the same way.  Single-process evaluation only.
    rank (not a reference argument): "hamming" (default) or "asymmetric" -- the ranking `exp=search rank=asymmetric` serves (DESIGN.md
    section 2.0): `test_codes` stay real-valued and every query pays its own |code|, quantised to `weight_bits` (4 or 8) bits, for a
    disagreeing bit of the sign-packed database.  Same triple, same limits; no tie bracket and no radii under it (ValueError), and
    single-process evaluation only (NotImplementedError for RowShards or a process group of more than one rank).
    rank="ternary", margin=m (not reference arguments): both code sets become ternary codes -- sign(x) where |x| > m, 0 otherwise -- and
    the ranking is ascending K = nbit - t_q . t_g, twice the matmul distance 0.5 (nbit - q g^T) on those codes: a
    bit either side is unsure of costs half a bit.  `margin` is required, finite and >= 0 (ValueError): there is no default, the scale of
    the codes belongs to the run.  No tie bracket and no radii (ValueError); single-process only (NotImplementedError), as "asymmetric".
    `threshold` is NOT this margin: the reference hands `ternary_threshold` to its un-vendored package, whose rule for it cannot be
    read, so threshold != 0 keeps raising NotImplementedError (the situation that made skip_queries_without_relevant a switch) and the
    ternary ranking is asked for by name.
    rank="cosine" | "euclidean" | "dot" (not reference arguments): the ranking of the real-valued codes themselves, before sign() --
    ascending 1 - cos, squared Euclidean distance or negated dot product; neither code set is binarised, so
    mAP under it minus the Hamming mAP is the run's quantisation gap.  Codes of 1 .. 256 finite dimensions (ValueError otherwise); no
    tie bracket and no radii (ValueError); single-process only (NotImplementedError).  `dist_metric` is NOT this switch, for the
    reason `threshold` is not the margin: dist_metric != "hamming" keeps raising NotImplementedError.
    shortlist=m with a dense rank (not a reference argument): the triple of the two-stage list `exp=search rank=<dense> shortlist=m`
    serves (`retrieval.evaluate_reranked`; DESIGN.md section 2.0, "two-stage") -- the first m rows by Hamming distance of the sign
    codes, ordered by the dense distance.  1 <= m <= 4096; R and every k must lie in [1, m] and R = -1 means m (ValueError otherwise);
    recall counts the relevant rows of the whole database.  The effective R and agreement@k with the exhaustive dense list are left
    in the module attribute `last_rerank`.  Under any other rank a shortlist is a ValueError."""
    global last_tie_bracket, last_hash_lookup, last_rerank, last_tie_expected
    if rank not in RANKS:
        raise ValueError(f"rank must be one of {RANKS}, got {rank!r}")
    if shortlist is not None:
        if rank not in DENSE_RANKS:
            raise ValueError(f"shortlist with rank='{rank}' is not built: a shortlist is reranked by a dense rank, one of {DENSE_RANKS}")
        shortlist = rt.check_shortlist(1, shortlist)[1]
    last_rerank = None
    if rank != "hamming" and (tie_bracket or radii is not None):
        raise ValueError(f"rank='{rank}' has no tie bracket and no radius lookup: both are defined on Hamming distances")
    if rank != "hamming" and tie_expected:
        raise ValueError(f"rank='{rank}' has no tie expectation: it is defined on Hamming distances, as the tie bracket is")
    if tie_expected and skip_queries_without_relevant:
        raise ValueError(rt.EXPECTED_NEEDS_ALL_QUERIES)
    if rank == "asymmetric" and int(weight_bits) not in rt.WEIGHT_BITS:
        raise ValueError(f"weight_bits must be one of {rt.WEIGHT_BITS}, got {weight_bits}")
    if rank == "ternary":
        margin = rt.check_margin(margin, "rank='ternary': margin")
    last_tie_bracket = None
    last_hash_lookup = None
    last_tie_expected = None
    _check(dist_metric, threshold, landmark_gt)
    ks = [int(k) for k in (PRs or [])]
    many = isinstance(R, (list, tuple)) or (hasattr(R, "__iter__") and not isinstance(R, (int, float)))
    Rs = [int(r) for r in R] if many else int(R)
    if many and not Rs:
        return [], [], []
    if rank != "hamming":     # neither tie bracket nor radii from here (refused above)
        res = _evaluate_ranked(rank, db_codes, db_labels, test_codes, test_labels, Rs, ks, remove_first_retrieved,
                               bool(skip_queries_without_relevant), weight_bits, margin, shortlist)
        if shortlist is not None:
            last_rerank = dict(metric=rank, shortlist=shortlist, R=res["R"], agreement=res["agreement"])
    else:
        res = _evaluate(db_codes, db_labels, test_codes, test_labels, Rs, ks, remove_first_retrieved, bool(skip_queries_without_relevant),
                        bool(tie_bracket), [int(r) for r in radii] if radii is not None else None, bool(tie_expected))
    if radii is not None:
        last_hash_lookup = dict({k: res[k] for k in ("precisions_radius", "recalls_radius", "retrieved_radius", "empty_radius")},
                                radii=[int(r) for r in radii])
    if tie_bracket:
        last_tie_bracket = {k: res[k] for k in ("mAP_low", "mAP_high", "precisions_low", "precisions_high", "recalls_low", "recalls_high")}
    if tie_expected:
        last_tie_expected = {k: res[k] for k in ("mAP_expected", "precisions_expected", "recalls_expected")}
    return res["mAP"], res["recalls"], res["precisions"]


def pr_curve_points(n_db: int) -> List[int]:
    """Retrieval depths of the P/R sweep: 1, 2, 5 decades up to the database size, plus the size itself."""
    pts, base = [], 1
    while base <= n_db:
        for m in (1, 2, 5):
            if base * m <= n_db:
                pts.append(base * m)
        base *= 10
    if not pts or pts[-1] != n_db:
        pts.append(n_db)
    return pts


def calculate_pr_curve(db_codes, db_labels, test_codes, test_labels, threshold=0., dist_metric="hamming",
                       remove_first_retrieved=False, Rs: Sequence[int] = None, rank="hamming"):
    """-> (recalls, precisions, Rs): mean precision / recall at each retrieval depth R (experiments/test_hashing.py:153-167).
    Every depth is a rank limit of ONE AP pass (16 limits per gallery scan): #relevant-in-top-R is that limit's `nrel`.
    rank (not a reference argument): "hamming" (default), or "cosine" | "euclidean" | "dot" -- the curve of the ranking of the
    real-valued codes (`calculate_mAP`); the other ranks of `calculate_mAP` have no curve here (ValueError)."""
    if rank != "hamming" and rank not in DENSE_RANKS:
        raise ValueError(f"rank must be 'hamming' or one of {DENSE_RANKS}, got {rank!r}")
    _check(dist_metric, threshold, None)
    if rank in DENSE_RANKS:
        _single_process(rank, db_codes, db_labels, test_codes, test_labels)
    n = db_codes.shape[0] - (1 if remove_first_retrieved else 0)
    Rs = [int(r) for r in (Rs if Rs is not None else pr_curve_points(max(n, 1)))]
    if not Rs:
        return [], [], []
    if rank in DENSE_RANKS:
        res = _evaluate_ranked(rank, db_codes, db_labels, test_codes, test_labels, Rs, [], remove_first_retrieved, False)
    else:
        res = _evaluate(db_codes, db_labels, test_codes, test_labels, Rs, [], remove_first_retrieved)
    total = res["total"].double()
    recalls, precisions = [], []
    for r, nrel in zip(Rs, res["nrel"]):
        nrel = nrel.double()
        precisions.append(float((nrel / r).mean().item()) if nrel.numel() else 0.0)
        recalls.append(float(torch.where(total > 0, nrel / total.clamp_min(1), torch.zeros_like(nrel)).mean().item())
                       if nrel.numel() else 0.0)
    return recalls, precisions, Rs


def get_hamm_dist(codes, centroids, normalize=True):
    """(B, nbit) codes vs (C, nbit) codebook -> (B, C) Hamming distance, divided by nbit when `normalize`
    (trainers/orthohash.py:362; in-repo twin get_hd, trainers/orthohash.py:263-264).  Output stays on the GPU."""
    dev = _device()
    a = rt.pack_sign(torch.as_tensor(codes).to(dev, torch.float32))
    b = rt.pack_sign(torch.as_tensor(centroids).to(dev, torch.float32))
    d = rt.hamming_dist(a, b).to(torch.float32)
    return d / codes.shape[1] if normalize else d


def get_sim(label_a, label_b, onehot=True):
    """Ground-truth similarity matrix (labels share >= 1 class) -- small-problem helper used by some reference losses."""
    if onehot:
        return (label_a.float() @ label_b.float().t() > 0).float()
    return (label_a.reshape(-1, 1) == label_b.reshape(1, -1)).float()
