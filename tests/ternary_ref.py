"""numpy reference of the ternary codes (csrc/hamming_ternary.hip): the ternariser, the two packed planes, the
distance K = nbit - t_q . t_g from the definition on UNPACKED int8 codes (never the popcount identity the kernels use -- that identity
is a separate function here, held against the definition by tests/test_ternary_cpu.py), top-k by a stable sort of (K, index), and the
AP integers through the brute force of tests/asymmetric_eval_ref.py (the fixed point floor(relrank 2^32 / rank))."""
import numpy as np

import asymmetric_eval_ref as aref


def ternarise(x, margin):
    """[rows, nbit] real codes -> int8 in {-1, 0, +1}: sign(x) where |x| > margin (compared as fp32, strictly), 0 otherwise; NaN -> 0"""
    x = np.asarray(x, dtype=np.float32)
    m = np.float32(margin)
    with np.errstate(invalid="ignore"):
        sure = np.abs(x) > m
        return np.where(sure & (x > 0), 1, np.where(sure, -1, 0)).astype(np.int8)


def _pack_bits(bits):
    """[rows, nbit] bool -> [rows, W] uint64, bit j of a row at bit j % 64 of word j // 64; bits past nbit are zero"""
    rows, nbit = bits.shape
    W = (nbit + 63) // 64
    padded = np.zeros((rows, W * 64), dtype=np.uint64)
    padded[:, :nbit] = bits
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(rows, W, 64) * weights).sum(-1, dtype=np.uint64)


def planes(t):
    """int8 ternary codes [rows, nbit] -> uint64 [rows, 2, W]: plane 0 = (t > 0), plane 1 = (t != 0)"""
    return np.stack([_pack_bits(t > 0), _pack_bits(t != 0)], axis=1)


def pack_sign(x, threshold=0.0):
    """the binary packer of the project: bit = (x - threshold) > 0 in fp32"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return _pack_bits((x - np.float32(threshold)) > 0)


def confidence_mask(x, margin):
    """retrieval.confidence_mask: pack_sign(x, margin) | pack_sign(-x, margin)"""
    x = np.asarray(x, dtype=np.float32)
    return pack_sign(x, margin) | pack_sign(-x, margin)


def dist(tq, tg):
    """K [Qn, G] int64 from the definition nbit - sum_j t_q,j t_g,j on unpacked codes"""
    tq, tg = np.asarray(tq, dtype=np.int64), np.asarray(tg, dtype=np.int64)
    return tq.shape[1] - tq @ tg.T


def dist_planes(pq, pg, nbit):
    """K by the identity nbit - popcount(mq & mg) + 2 popcount((sq ^ sg) & mq & mg) on packed planes (what the kernels compute)"""
    def pop(a):
        return np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=-1).sum(-1, dtype=np.int64)
    both = pq[:, None, 1, :] & pg[None, :, 1, :]
    return nbit - pop(both) + 2 * pop((pq[:, None, 0, :] ^ pg[None, :, 0, :]) & both)


def topk(K, k, base=0):
    """ascending (K, index), stable: (idx int64 [Qn, k], dist int64 [Qn, k]); -1 past the gallery"""
    Qn, G = K.shape
    idx = np.full((Qn, k), -1, np.int64)
    dst = np.full((Qn, k), -1, np.int64)
    order = np.argsort(K, axis=1, kind="stable")[:, :k]
    n = order.shape[1]
    idx[:, :n] = order + base
    dst[:, :n] = np.take_along_axis(K, order, axis=1)
    return idx, dst


def evaluate(K, q_labels, g_labels, limits, remove_first=False):
    """(S uint64 [n, Qn], nrel int64 [n, Qn], total int64 [Qn]) of the ranking by ascending (K, index)"""
    return aref.evaluate(K, aref.relevance(q_labels, g_labels), limits, remove_first)


def summarize(S, nrel, total, nR, ks):
    """float64 mAP per R, P@k and R@k per k from the integers of `evaluate` whose limits were the nR values of R, then ks"""
    S, nrel, total = S.astype(np.float64), nrel.astype(np.float64), total.astype(np.float64)
    ap = np.where(nrel[:nR] > 0, S[:nR] / (np.maximum(nrel[:nR], 1) * 4294967296.0), 0.0)
    hits = nrel[nR:]
    prec = [float((hits[t] / k).mean()) for t, k in enumerate(ks)]
    rec = [float(np.where(total > 0, hits[t] / np.maximum(total, 1), 0.0).mean()) for t in range(len(ks))]
    return [float(a.mean()) for a in ap], prec, rec
