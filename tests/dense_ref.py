"""numpy / fp64 reference of the rankings of real-valued codes ("real-valued codes"; csrc/dense_rank.hip):
the three distances from their definitions, the order key, brute-force top-k, bounds on what the kernels' fp32 chains may differ from
the fp64 distances by, and the bracket of AP over every ranking those bounds allow.

Error bounds.  u = 2^-24 (fp32 unit roundoff); the codes are fp32 numbers, so the fp64 distances below are exact up to fp64 rounding
(2^-53, ignored).  gamma_m = m u / (1 - m u) <= (m + 1) u as long as m (m + 1) u <= 1, which holds for m <= 4000.

* dot.  acc = fmaf(q_j, g_j, acc) over n terms, one rounding each: |acc - q.g| <= gamma_n sum_j |q_j g_j| (Higham, Accuracy and
  Stability of Numerical Algorithms, section 3.1, with the product exact inside the fma).  Negation and + 0.0f are exact:
      E = (n + 1) u sum_j |q_j g_j|.
* euclidean.  t_j = fl(q_j - g_j) = (q_j - g_j)(1 + d), |d| <= u, so t_j^2 = (q_j - g_j)^2 (1 + d)^2; the n fmaf steps add terms that are
  all >= 0, so the result is D (1 + theta), |theta| <= (1 + u)^(n + 2) - 1 <= gamma_(n + 2):
      E = (n + 3) u D.
* cosine.  Per row: s = sum of squares by n fmaf steps = |x|^2 (1 + theta_n); sqrt halves that relative error and adds u; the
  division adds u; the product x_j * inv adds u: every entry of the fp32 x^ has relative error at most e = (n / 2 + 3) u + O(u^2).
  The fp32 chain on those entries errs by gamma_n sum_j |q^_j g^_j| (1 + e)^2, the perturbed entries move the sum by at most
  ((1 + e)^2 - 1) sum_j |q^_j g^_j|, and sum_j |q^_j g^_j| <= 1 (Cauchy-Schwarz on unit vectors); 1.0f - acc rounds once on a result
  of magnitude <= 2.  Together n u + (n + 6) u + 2 u = (2 n + 8) u to first order; the bound used leaves the second-order terms
  more than enough room:
      E = (3 n + 10) u.
"""
import numpy as np

METRICS = ("cosine", "euclidean", "dot")
U = 2.0 ** -24


def normalise(x):
    """fp64 rows scaled to unit length; a zero row stays zero"""
    x = np.asarray(x, np.float64)
    s = np.sqrt((x * x).sum(1, keepdims=True))
    return np.where(s > 0, x / np.where(s > 0, s, 1.0), 0.0)


def dist(q, g, metric):
    """[Qn, n], [G, n] -> fp64 [Qn, G] from the definitions (+ 0.0: no negative zero)"""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    if metric == "dot":
        return -(q @ g.T) + 0.0
    if metric == "euclidean":
        return ((q[:, None, :] - g[None, :, :]) ** 2).sum(-1) + 0.0
    if metric == "cosine":
        return (1.0 - normalise(q) @ normalise(g).T) + 0.0
    raise ValueError(metric)


def bound(q, g, metric):
    """fp64 [Qn, G]: E with |D_fp32 - D_fp64| <= E (module docstring)"""
    q, g = np.asarray(q, np.float64), np.asarray(g, np.float64)
    n = q.shape[1]
    if metric == "dot":
        return (n + 1) * U * (np.abs(q) @ np.abs(g).T)
    if metric == "euclidean":
        return (n + 3) * U * dist(q, g, metric)
    if metric == "cosine":
        return np.full((q.shape[0], g.shape[0]), (3 * n + 10) * U)
    raise ValueError(metric)


def order_key(D32):
    """ord(D) of fp32 distances as uint64 values in [0, 2^32): b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), b = bits(D + 0.0f)"""
    b = (np.asarray(D32, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    return np.where(b >> np.uint64(31) != 0, b ^ np.uint64(0xFFFFFFFF), b ^ np.uint64(0x80000000))


def bits(x32):
    return np.ascontiguousarray(np.asarray(x32, np.float32)).view(np.uint32)


def topk(D, k, base=0):
    """ascending (D, index) -> (idx int64 [Qn, k], dist float32 [Qn, k]); -1 / +inf past the gallery"""
    Qn, G = D.shape
    idx = np.full((Qn, k), -1, np.int64)
    d = np.full((Qn, k), np.inf, np.float32)
    index = np.arange(G)
    for i in range(Qn):
        o = np.lexsort((index, D[i]))[:k]
        idx[i, :o.size] = o + base
        d[i, :o.size] = D[i, o]
    return idx, d


def merge_lists(idx_lists, dist_lists, k):
    """per-shard (idx, dist) lists -> the k first by ascending (ord(dist), idx), empty slots (-1) last"""
    idx, d = np.concatenate(idx_lists, 1), np.concatenate(dist_lists, 1)
    out_i, out_d = np.full((idx.shape[0], k), -1, np.int64), np.full((idx.shape[0], k), np.inf, np.float32)
    for i in range(idx.shape[0]):
        keep = np.flatnonzero(idx[i] >= 0)
        o = keep[np.lexsort((idx[i, keep], order_key(d[i, keep])))][:k]
        out_i[i, :o.size], out_d[i, :o.size] = idx[i, o], d[i, o]
    return out_i, out_d


def _ap(rel_in_order):
    pos = np.flatnonzero(rel_in_order) + 1
    return float((np.arange(1, pos.size + 1) / pos).mean()) if pos.size else 0.0


def ap_bracket(D, E, rel):
    """Per query (AP_low, AP_high) over every ranking the bounds allow: rows in fp64 order; adjacent rows whose gap is <= E_a + E_b are
    chained into groups; AP_high puts each group's relevant rows first, AP_low last.  -> two fp64 [Qn] arrays"""
    Qn, G = D.shape
    lo, hi = np.zeros(Qn), np.zeros(Qn)
    index = np.arange(G)
    for i in range(Qn):
        o = np.lexsort((index, D[i]))
        d, e, r = D[i, o], E[i, o], rel[i, o]
        new = np.r_[True, (d[1:] - d[:-1]) > (e[1:] + e[:-1])]
        group = np.cumsum(new) - 1
        hi[i] = _ap(r[np.lexsort((~r, group))])
        lo[i] = _ap(r[np.lexsort((r, group))])
    return lo, hi


def hamming(q, g):
    """[Qn, n], [G, n] real codes -> int64 [Qn, G] Hamming distances of their signs (x > 0)"""
    return ((np.asarray(q) > 0)[:, None, :] != (np.asarray(g) > 0)[None, :, :]).sum(-1).astype(np.int64)
