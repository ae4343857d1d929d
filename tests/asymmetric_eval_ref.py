"""numpy reference of the evaluation under the weighted (asymmetric) ranking: brute force on the full distance
matrix of tests/weighted_topk_ref.py -- the ranking by np.lexsort((index, D)), remove_first by dropping rank 1 of that order, the
fixed-point AP terms floor(relrank 2^32 / rank) in Python integers -- and a numpy restatement of the rank-count identity the kernels of
csrc/hamming_rankcount.hip implement, which tests/test_asymmetric_eval_cpu.py holds against the brute force."""
import numpy as np

import weighted_topk_ref as wref

ALL = 0xFFFFFFFF


def relevance(q_labels, g_labels):
    """[Qn, G] bool: equal ids (1-D labels) or intersecting indicator rows (2-D, multi-hot)"""
    q_labels, g_labels = np.asarray(q_labels), np.asarray(g_labels)
    if q_labels.ndim == 1:
        return q_labels[:, None] == g_labels[None, :]
    return ((q_labels != 0).astype(np.int64) @ (g_labels != 0).astype(np.int64).T) > 0


def distances(codes, g, bits, mask=None):
    """[Qn, nbit] fp32 real-valued query codes, [G, W] uint64 gallery -> int64 [Qn, G] weighted distances"""
    return wref.dist(wref.pack_sign(codes), g, wref.weights(codes, bits, mask))


def _limit(r):
    return ALL if int(r) <= 0 else int(r)


def account(ranks, limits):
    """1-based ranks of one query's relevant rows in ranking order (after remove_first) -> (S, nrel) per limit"""
    S, nrel = [0] * len(limits), [0] * len(limits)
    for relrank, rank in enumerate(ranks, start=1):
        term = (relrank << 32) // int(rank)
        for t, lim in enumerate(limits):
            if rank <= lim:
                S[t] += term
                nrel[t] += 1
    return S, nrel


def evaluate(D, rel, limits, remove_first=False):
    """Brute force.  D int64 [Qn, G], rel bool [Qn, G], limits: rank limits (<= 0 = all)
    -> S uint64 [n, Qn], nrel int64 [n, Qn], total int64 [Qn] (relevant rows, less a dropped relevant rank-1 row)"""
    Qn, G = D.shape
    lims = [_limit(r) for r in limits]
    S = np.zeros((len(lims), Qn), np.uint64)
    nrel = np.zeros((len(lims), Qn), np.int64)
    total = np.zeros(Qn, np.int64)
    index = np.arange(G)
    for i in range(Qn):
        order = np.lexsort((index, D[i]))
        if remove_first:
            order = order[1:]
        r = rel[i, order]
        total[i] = int(r.sum())
        s, n = account(np.flatnonzero(r) + 1, lims)
        S[:, i] = np.array(s, dtype=np.uint64)
        nrel[:, i] = n
    return S, nrel, total


def evaluate_by_rank_count(D, rel, limits, remove_first=False, base=0):
    """The same integers by the rank-count identity: key = D << 32 | global index; r_0 < ... < r_{n-1} the sorted keys of the relevant
    rows; bins[#{j : r_j < key(row)}] += 1 over all rows; rank(r_j) = sum_{b <= j} bins[b], rank among relevant rows j + 1; bin n is not
    read.  remove_first: frel = rank(r_0) == 1; a relevant row at rank 1 is skipped, every other row uses rank - 1 and relrank - frel."""
    Qn, G = D.shape
    lims = [_limit(r) for r in limits]
    S = np.zeros((len(lims), Qn), np.uint64)
    nrel = np.zeros((len(lims), Qn), np.int64)
    total = np.zeros(Qn, np.int64)
    for i in range(Qn):
        keys = (D[i].astype(np.uint64) << np.uint64(32)) | (np.arange(G, dtype=np.uint64) + np.uint64(base))
        r = np.sort(keys[rel[i]])
        n = r.size
        if n == 0:
            continue
        bins = np.bincount(np.searchsorted(r, keys, side="left"), minlength=n + 1)
        rank = np.cumsum(bins[:n])
        frel = int(rank[0] == 1)
        s = [0] * len(lims)
        c = [0] * len(lims)
        for j in range(n):
            rk, rr = int(rank[j]), j + 1
            if remove_first:
                if rk == 1:
                    continue
                rk, rr = rk - 1, rr - frel
            term = (rr << 32) // rk
            for t, lim in enumerate(lims):
                if rk <= lim:
                    s[t] += term
                    c[t] += 1
        S[:, i] = np.array(s, dtype=np.uint64)
        nrel[:, i] = c
        total[i] = n - (frel if remove_first else 0)
    return S, nrel, total


def clustered_codes(rng, rows, nbit, labels, centres, noise=0.78):
    """class centres +-1 plus N(0, noise^2): the real-valued codes of a trained model (about 10 % sign flips at 0.78)"""
    return (centres[labels] + noise * rng.standard_normal((rows, nbit))).astype(np.float32)
