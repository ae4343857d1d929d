"""Plain numpy / Python restatement of the tie bracket -- shared by tests/test_tie_bracket_cpu.py and
tests/test_tie_bracket_gpu.py; not a test itself.

For one query, bucket d (ascending Hamming distance) holds n_d gallery rows of which r_d are relevant.  A tie order is any ranking
that ascends in distance; inside a bucket the order is free.  `bracket_one` gives the smallest / largest AP@R over all tie orders in
closed form -- as float64 (`exact=False`) or as the project's integers S = sum floor(relrank * 2^32 / rank), nrel (`exact=True`,
what ch_hamming_tie_bracket must reproduce bit for bit); `brute_force` enumerates the orders of a tiny problem.
"""
from __future__ import annotations

import itertools

import numpy as np

TWO32 = 1 << 32


def ap_value(S, nrel, exact=True):
    """AP of a candidate: the float64 that retrieval.ap_from_fixed computes (exact) or the plain ratio"""
    if not nrel:
        return 0.0
    return float(S) / float(nrel * TWO32) if exact else S / nrel


def run_sum(rel0, rank0, cnt, exact=True):
    """sum over i < cnt of term(rel0 + i + 1, rank0 + i + 1): cnt relevant rows on consecutive ranks from rank0 + 1"""
    if cnt <= 0:
        return 0 if exact else 0.0
    i = np.arange(1, cnt + 1, dtype=np.uint64)
    if exact:       # relrank < 2^32, so relrank << 32 fits 64 bits and the floor division is exact
        return int((((np.uint64(rel0) + i) << np.uint64(32)) // (np.uint64(rank0) + i)).sum(dtype=np.uint64))
    return float(sum((rel0 + k) / (rank0 + k) for k in range(1, cnt + 1)))


def _walk(buckets, R, exact):
    """buckets: [(n, r)] ascending distance; -> (S_low, nrel_low, S_high, nrel_high) for rank limit R (<= 0: none)"""
    B = K = 0
    SH = SL = 0 if exact else 0.0
    for n, r in buckets:
        if n == 0:
            continue
        if 0 < R < B + n:            # the bucket the limit cuts: `take` of its rows are ranked, t of them relevant
            take = R - B
            tmin, tmax = max(0, take - (n - r)), min(r, take)
            best = worst = None
            for t in range(tmin, tmax + 1):
                hi = SH + run_sum(K, B, t, exact)                   # the t relevant rows lead the bucket
                lo = SL + run_sum(K, B + take - t, t, exact)        # ... or close the `take` positions
                if best is None or ap_value(hi, K + t, exact) > ap_value(best[0], best[1], exact):
                    best = (hi, K + t)                              # equal values keep the smaller t
                if worst is None or ap_value(lo, K + t, exact) < ap_value(worst[0], worst[1], exact):
                    worst = (lo, K + t)
            return worst[0], worst[1], best[0], best[1]
        SH += run_sum(K, B, r, exact)                               # whole bucket inside: relevant rows first ...
        SL += run_sum(K, B + (n - r), r, exact)                     # ... or last
        B += n
        K += r
    return SL, K, SH, K


def bracket_one(buckets, R, remove_first=False, exact=True):
    """-> (S_low, nrel_low, S_high, nrel_high).  remove_first: rank 1 of the tie order is dropped -- any row of the lowest non-empty
    bucket; dropping an irrelevant row is tried first and dropping a relevant one replaces it only where strictly better."""
    buckets = [(int(n), int(r)) for n, r in buckets]
    if not remove_first:
        return _walk(buckets, R, exact)
    d0 = next((d for d, (n, _) in enumerate(buckets) if n > 0), None)
    if d0 is None:
        return _walk(buckets, R, exact)
    n0, r0 = buckets[d0]
    res = None
    if n0 > r0:
        res = _walk(buckets[:d0] + [(n0 - 1, r0)] + buckets[d0 + 1:], R, exact)
    if r0 > 0:
        alt = _walk(buckets[:d0] + [(n0 - 1, r0 - 1)] + buckets[d0 + 1:], R, exact)
        if res is None:
            res = alt
        else:
            lo = alt[:2] if ap_value(alt[0], alt[1], exact) < ap_value(res[0], res[1], exact) else res[:2]
            hi = alt[2:] if ap_value(alt[2], alt[3], exact) > ap_value(res[2], res[3], exact) else res[2:]
            res = tuple(lo) + tuple(hi)
    return res


def bracket_from_counts(counts, limits, remove_first=False):
    """counts [Qn, nb, 2] -> (S_low uint64 [n, Qn], nrel_low uint32, S_high, nrel_high): the integers of ch_hamming_tie_bracket"""
    counts = np.asarray(counts)
    Qn = counts.shape[0]
    S_lo = np.zeros((len(limits), Qn), dtype=np.uint64)
    S_hi = np.zeros_like(S_lo)
    n_lo = np.zeros((len(limits), Qn), dtype=np.uint32)
    n_hi = np.zeros_like(n_lo)
    for qi in range(Qn):
        b = [(int(n), int(r)) for n, r in counts[qi]]
        for li, R in enumerate(limits):
            S_lo[li, qi], n_lo[li, qi], S_hi[li, qi], n_hi[li, qi] = bracket_one(b, int(R), remove_first, True)
    return S_lo, n_lo, S_hi, n_hi


def ap_from_fixed(S, nrel):
    S, nrel = np.asarray(S), np.asarray(nrel)
    return np.where(nrel > 0, S.astype(np.float64) / (np.maximum(nrel, 1).astype(np.float64) * float(TWO32)), 0.0)


def hits_extremes(buckets, k, remove_first=False):
    """-> (hits_low, hits_high, recall_low, recall_high) at depth k: the extreme numbers of relevant rows of the bucket k cuts"""
    def one(bk):
        B = lo = hi = 0
        for n, r in bk:
            take = min(max(k - B, 0), n)
            hi += min(r, take)
            lo += max(0, take - (n - r))
            B += n
        tot = sum(r for _, r in bk)
        return lo, hi, (lo / tot if tot else 0.0), (hi / tot if tot else 0.0)
    buckets = [(int(n), int(r)) for n, r in buckets]
    d0 = next((d for d, (n, _) in enumerate(buckets) if n > 0), None)
    if not remove_first or d0 is None:
        return one(buckets)
    n0, r0 = buckets[d0]
    got = []
    if n0 > r0:
        got.append(one(buckets[:d0] + [(n0 - 1, r0)] + buckets[d0 + 1:]))
    if r0 > 0:
        got.append(one(buckets[:d0] + [(n0 - 1, r0 - 1)] + buckets[d0 + 1:]))
    return min(x[0] for x in got), max(x[1] for x in got), min(x[2] for x in got), max(x[3] for x in got)


def counts_from_codes(q, g, q_labels, g_labels):
    """packed uint64 codes + labels (1-D ids or 2-D multi-hot) -> bucket counts [Qn, 64W+1, 2] uint32"""
    q, g = np.asarray(q, dtype=np.uint64), np.asarray(g, dtype=np.uint64)
    Qn, W = q.shape
    nb = 64 * W + 1
    x = q[:, None, :] ^ g[None, :, :]
    dist = np.unpackbits(x.view(np.uint8), axis=-1).reshape(Qn, g.shape[0], -1).sum(-1)
    ql, gl = np.asarray(q_labels), np.asarray(g_labels)
    rel = (ql[:, None] == gl[None, :]) if ql.ndim == 1 else ((ql.astype(np.int64) @ gl.astype(np.int64).T) > 0)
    counts = np.zeros((Qn, nb, 2), dtype=np.uint32)
    for qi in range(Qn):
        counts[qi, :, 0] = np.bincount(dist[qi], minlength=nb)
        counts[qi, :, 1] = np.bincount(dist[qi][rel[qi]], minlength=nb)
    return counts


def _ap_of_order(rel_flags, R):
    """AP@R of one ranking given as relevance flags; R <= 0: no limit"""
    lim = len(rel_flags) if R <= 0 else min(R, len(rel_flags))
    s, k = 0.0, 0
    for rank in range(1, lim + 1):
        if rel_flags[rank - 1]:
            k += 1
            s += k / rank
    return s / k if k else 0.0


def brute_force(buckets, R, remove_first=False, k=None):
    """Every permutation inside every bucket (equal relevance patterns once), and with remove_first the drop of that order's rank 1:
    -> (AP_min, AP_max), or with k the (min, max) number of relevant rows in the top k and of hits / total."""
    per_bucket = []
    for n, r in buckets:
        flags = (1,) * int(r) + (0,) * (int(n) - int(r))
        per_bucket.append(sorted(set(itertools.permutations(flags))))
    lo, hi = None, None
    rlo, rhi = None, None
    for combo in itertools.product(*per_bucket):
        order = [f for part in combo for f in part]
        if remove_first:
            order = order[1:]
        if k is None:
            v = _ap_of_order(order, R)
        else:
            v = sum(order[:k])
            tot = sum(order)
            rv = v / tot if tot else 0.0
            rlo, rhi = (rv if rlo is None else min(rlo, rv)), (rv if rhi is None else max(rhi, rv))
        lo, hi = (v if lo is None else min(lo, v)), (v if hi is None else max(hi, v))
    return (lo, hi) if k is None else (lo, hi, rlo, rhi)
