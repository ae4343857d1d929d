"""numpy reference of the two-stage search ("two-stage"): a Hamming shortlist of the sign codes, ordered by a
dense distance of the real-valued codes -- shared by tests/test_rerank_cpu.py and tests/test_rerank_gpu.py; not a test itself.

The shortlist S_m(q) is `ranked_ref.ranked` (the stable argsort of the full Hamming matrix, cut at m, cut by a radius); D is a full
distance matrix, `dense_ref.dist` unless the caller brings its own; the order is np.lexsort((index, D)) over the shortlist.
"""
import numpy as np

import asymmetric_eval_ref as aref
import dense_ref as dref
import ranked_ref as rref


def pack(x):
    """[rows, n] real codes -> packed uint64 [rows, ceil(n / 64)] sign codes (bit j = x_j > 0, little endian)"""
    b = (np.asarray(x) > 0).astype(np.uint8)
    pad = -b.shape[1] % 64
    if pad:
        b = np.concatenate([b, np.zeros((b.shape[0], pad), np.uint8)], 1)
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view("<u8")


def shortlist(xq, xg, m, radius=None):
    """int64 [Qn, m]: the first min(m, G) rows by ascending (Hamming distance, index), -1 behind them and behind the radius"""
    return rref.ranked(pack(xq), pack(xg), m, radius=radius)[0]


def rerank(D, cand, k, base=0):
    """D [Qn, G] distances, cand int64 [Qn, m] global ids (row = id - base; id < 0: an empty slot) -> (idx int64 [Qn, k], dist fp32
    [Qn, k]): the candidates by ascending (D, index), -1 / +inf past the filled slots.  A row listed twice appears twice."""
    Qn = cand.shape[0]
    idx = np.full((Qn, k), -1, np.int64)
    d = np.full((Qn, k), np.inf, np.float32)
    for i in range(Qn):
        rows = cand[i][cand[i] >= 0] - base
        o = rows[np.lexsort((rows, D[i, rows]))][:k]
        idx[i, :o.size] = o + base
        d[i, :o.size] = D[i, o]
    return idx, d


def two_stage(xq, xg, metric, m, k, radius=None, D=None):
    """the two-stage list from the definitions"""
    D = dref.dist(xq, xg, metric) if D is None else D
    return rerank(D, shortlist(xq, xg, m, radius), k)


def evaluate(D, cand, rel, limits, remove_first=False):
    """Brute force of the evaluation of the two-stage list, row by row: the list is the shortlist in (D, index) order and nothing else
    -- no row outside it has a rank -- remove_first drops its rank 1, the AP terms are `asymmetric_eval_ref.account`'s
    floor(relrank 2^32 / rank) in Python integers, and `total` counts the relevant rows of the WHOLE gallery (less a dropped relevant
    rank-1 row).  -> S uint64 [n, Qn], nrel int64 [n, Qn], total int64 [Qn]"""
    Qn = D.shape[0]
    lims = [int(r) for r in limits]
    S = np.zeros((len(lims), Qn), np.uint64)
    nrel = np.zeros((len(lims), Qn), np.int64)
    total = np.zeros(Qn, np.int64)
    for i in range(Qn):
        rows = cand[i][cand[i] >= 0]
        order = rows[np.lexsort((rows, D[i, rows]))]
        total[i] = int(rel[i].sum())
        if remove_first and order.size:
            total[i] -= int(rel[i, order[0]])
            order = order[1:]
        s, n = aref.account(np.flatnonzero(rel[i, order]) + 1, lims)
        S[:, i] = np.array(s, dtype=np.uint64)
        nrel[:, i] = n
    return S, nrel, total


def agreement(full_idx, two_idx, k):
    """mean share of the exhaustive top-k (full_idx [Qn, >= k]) found in the two-stage top-k"""
    shares = []
    for a, b in zip(full_idx[:, :k], two_idx[:, :k]):
        a = a[a >= 0]
        shares.append(np.isin(a, b[b >= 0]).sum() / max(a.size, 1))
    return float(np.mean(shares))
