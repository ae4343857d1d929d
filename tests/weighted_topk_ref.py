"""numpy reference of the weighted (asymmetric) Hamming ranking: the quantisation rule in fp64, the distance as
an integer matrix product of the differing bits with the weights, the ranking by np.lexsort((index, D)).  Packed words are uint64,
bit i of word w = code bit 64 w + i (little endian), as `retrieval.pack_sign` writes them."""
import numpy as np


def bits_of(x):
    """[..., W] uint64 -> [..., 64 W] {0,1}"""
    x = np.ascontiguousarray(x)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape[:-1] + (x.shape[-1] * 8,)), axis=-1, bitorder="little")


def pack_bits(b):
    """[..., 64 W] {0,1} -> [..., W] uint64"""
    b = np.ascontiguousarray(b.astype(np.uint8))
    return np.packbits(b, axis=-1, bitorder="little").view(np.uint64)


def pack_sign(codes):
    """[rows, nbit] fp32 -> [rows, W] uint64, bit = code > 0, bits past nbit zero"""
    rows, nbit = codes.shape
    W = (nbit + 63) // 64
    b = np.zeros((rows, 64 * W), np.uint8)
    b[:, :nbit] = codes > 0
    return pack_bits(b)


def weights(codes, bits, mask=None):
    """[Qn, nbit] fp32 (+ mask uint64 [W] or [Qn, W]) -> int64 [Qn, 64 W]: w = floor(a L / amax + 0.5) in fp64, a = |c| or 0 where c is
    not finite or the mask clears the bit; all zero when amax = 0; zero past nbit"""
    codes = np.asarray(codes, np.float32)
    Qn, nbit = codes.shape
    W = (nbit + 63) // 64
    L = float((1 << bits) - 1)
    a = np.zeros((Qn, 64 * W), np.float64)
    a[:, :nbit] = np.abs(codes.astype(np.float64))
    a[~np.isfinite(a)] = 0.0
    if mask is not None:
        keep = bits_of(np.broadcast_to(mask if mask.ndim == 2 else mask[None, :], (Qn, W)))
        a[keep == 0] = 0.0
    amax = a.max(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.floor(a * L / amax + 0.5)
    w[np.broadcast_to(amax == 0.0, w.shape)] = 0.0
    return w.astype(np.int64)


def planes_of(w, bits):
    """int64 [Qn, 64 W] -> uint64 [Qn, bits, W]: bit b of planes[i, p, t] = bit p of w[i, 64 t + b]"""
    return np.stack([pack_bits((w >> p) & 1) for p in range(bits)], axis=1)


def dist(q, g, w):
    """[Qn, W], [G, W] uint64, w int64 [Qn, 64 W] -> int64 [Qn, G]: D = ((q ^ g) bits) @ w"""
    gb = bits_of(g).astype(np.int64)                                  # [G, 64 W]
    qb = bits_of(q).astype(np.int64)
    out = np.empty((q.shape[0], g.shape[0]), np.int64)
    for i in range(q.shape[0]):
        out[i] = (gb ^ qb[i][None, :]) @ w[i]
    return out


def topk(D, k, base=0):
    """ascending (D, index); -1 past the end of the gallery -> (idx int64 [Qn, k], dist int32 [Qn, k])"""
    Qn, G = D.shape
    idx = np.full((Qn, k), -1, np.int64)
    dst = np.full((Qn, k), -1, np.int32)
    n = min(k, G)
    index = np.arange(G)
    for i in range(Qn):
        order = np.lexsort((index, D[i]))[:n]
        idx[i, :n] = order + base
        dst[i, :n] = D[i, order]
    return idx, dst


def tied_at_k(D, k):
    """share of queries whose k-th hit ties with a row left out"""
    s = np.sort(D, axis=1)
    return float((s[:, k - 1] == s[:, k]).mean()) if D.shape[1] > k else 0.0
