"""numpy reference of filtered search ("filtered search"): brute force over the full distance matrix -- the rows
that are not admitted are removed, the rest is stably ordered by (distance, global index) and cut at k, with a -1 tail.  The distances
are the existing references' (weighted_topk_ref.dist: plain = every weight 1, masked = the mask's bits as weights, weighted = the
quantised weights; ternary_ref.dist_planes), not a restatement."""
import numpy as np

import ternary_ref as tref
import weighted_topk_ref as wref


def pack_allow(allow, garbage=False):
    """bool [G] -> uint64 [ceil(G / 64)], bit r & 63 of word r >> 6 = allow[r]; garbage: ones in every bit past G"""
    allow = np.asarray(allow, bool)
    G = allow.shape[0]
    bits = np.full(((G + 63) // 64) * 64, bool(garbage))
    bits[:G] = allow
    return wref.pack_bits(bits.astype(np.uint8))


def admitted(Qn, G, allow=None, group=None, want=None, exclude=False, base=0):
    """bool [Qn, G]: row r is admitted for query i iff (allow is None or allow[r]) and (want is None or want[i] < 0 or
    (grp(r) == want[i]) != exclude), grp(r) = group[r], or base + r without a group plane"""
    adm = np.ones((Qn, G), bool)
    if allow is not None:
        adm &= np.asarray(allow, bool)[None, :]
    if want is not None:
        want = np.asarray(want, np.int64)
        grp = np.asarray(group, np.int64) if group is not None else base + np.arange(G, dtype=np.int64)
        part = (grp[None, :] == want[:, None]) != bool(exclude)
        adm &= part | (want < 0)[:, None]
    return adm


def topk(D, adm, k, base=0):
    """(idx int64 [Qn, k], dist int32 [Qn, k]): per query the admitted rows by ascending (D, index), cut at k, -1 behind them"""
    Qn, G = D.shape
    idx = np.full((Qn, k), -1, np.int64)
    dst = np.full((Qn, k), -1, np.int32)
    for i in range(Qn):
        rows = np.flatnonzero(adm[i])
        order = rows[np.argsort(D[i, rows], kind="stable")][:k]
        idx[i, :order.size] = order + base
        dst[i, :order.size] = D[i, order]
    return idx, dst


def hamming(q, g, mask=None):
    """plain / masked Hamming distances [Qn, G] int64 of packed uint64 codes: weighted_topk_ref.dist under 0 / 1 weights"""
    Qn, W = q.shape
    if mask is None:
        w = np.ones((Qn, 64 * W), np.int64)
    else:
        w = wref.bits_of(np.broadcast_to(mask if mask.ndim == 2 else mask[None, :], (Qn, W))).astype(np.int64)
    return wref.dist(q, g, w)


def weighted(q, g, w):
    return wref.dist(q, g, w)


def ternary(pq, pg, nbit):
    return tref.dist_planes(pq, pg, nbit)
