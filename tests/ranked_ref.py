"""Plain numpy restatement of ranked lists of any depth, radius search and hash lookup -- shared by
tests/test_ranked_cpu.py and tests/test_ranked_gpu.py; not a test itself.

The ranking is the stable argsort of the full distance matrix (oracle.hamming_oracle.dist): ascending (distance, gallery index).  The
kernels never build that matrix; they count, prefix and scatter (csrc/hamming_rank.hip) -- another algorithm, the same integers.
"""
import numpy as np

from oracle import hamming_oracle as ho


def ranking(q, g, mask=None):
    """-> (order int64 [Qn, G], sorted distances int32 [Qn, G], distance matrix int32 [Qn, G]); mask: uint64 [W] shared by all queries"""
    q = np.ascontiguousarray(q, dtype=np.uint64)
    g = np.ascontiguousarray(g, dtype=np.uint64)
    if mask is not None:
        m = np.asarray(mask).astype(np.uint64)
        q, g = q & m[None, :], g & m[None, :]
    d = ho.dist(q, g) if g.shape[0] and q.shape[0] else np.zeros((q.shape[0], g.shape[0]), dtype=np.int32)
    order = np.argsort(d, axis=1, kind="stable").astype(np.int64)
    return order, np.take_along_axis(d, order, axis=1).astype(np.int32), d


def ranked(q, g, k, g_index_base=0, radius=None, mask=None):
    """(idx int64 [Qn, k], dist int32 [Qn, k]): the first k of the ranking, -1 past min(k, G) and, with a radius, past dist <= radius"""
    order, ds, _ = ranking(q, g, mask)
    Qn, G = order.shape
    idx = np.full((Qn, k), -1, dtype=np.int64)
    dist = np.full((Qn, k), -1, dtype=np.int32)
    n = min(k, G)
    idx[:, :n] = order[:, :n] + g_index_base
    dist[:, :n] = ds[:, :n]
    if radius is not None:
        far = dist > radius
        idx[far] = -1
        dist[far] = -1
    return idx, dist


def radius_csr(q, g, radius, g_index_base=0, mask=None, max_hits=None):
    """(offsets int64 [Qn + 1], idx int64 [total], dist int32 [total]): per query the rows with dist <= radius in ranking order"""
    order, ds, _ = ranking(q, g, mask)
    offsets, idx, dist = [0], [], []
    for i in range(order.shape[0]):
        n = int((ds[i] <= radius).sum())
        if max_hits is not None:
            n = min(n, max_hits)
        idx.append(order[i, :n] + g_index_base)
        dist.append(ds[i, :n])
        offsets.append(offsets[-1] + n)
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, dtype=t)
    return np.asarray(offsets, dtype=np.int64), cat(idx, np.int64), cat(dist, np.int32)


def relevance(q_labels, g_labels):
    """bool [Qn, G]: 1-D class ids are relevant when equal, 2-D indicator rows when they share a class"""
    q_labels, g_labels = np.asarray(q_labels), np.asarray(g_labels)
    if q_labels.ndim == 1:
        return q_labels[:, None] == g_labels[None, :]
    return (q_labels.astype(np.int64) @ g_labels.astype(np.int64).T) > 0


def bucket_counts2(d, rel, nb):
    """distance matrix + relevance -> [Qn, nb, 2] int64 (rows, relevant rows) per (query, distance), counted row by row"""
    out = np.zeros((d.shape[0], nb, 2), dtype=np.int64)
    for i in range(d.shape[0]):
        np.add.at(out[i, :, 0], d[i], 1)
        np.add.at(out[i, :, 1], d[i], rel[i].astype(np.int64))
    return out


def hash_lookup(d, rel, radii, remove_first=False):
    """Brute force on the distance matrix: -> dict(retrieved int64 [Qn, nr], hits int64 [Qn, nr], precisions, recalls, retrieved_mean,
    empty: float64 [nr]).  remove_first: each query's rank-1 row (smallest (distance, index)) is dropped before anything is counted."""
    Qn, G = d.shape
    retrieved = np.zeros((Qn, len(radii)), dtype=np.int64)
    hits = np.zeros((Qn, len(radii)), dtype=np.int64)
    P = np.zeros((Qn, len(radii)))
    R = np.zeros((Qn, len(radii)))
    for i in range(Qn):
        keep = np.ones(G, dtype=bool)
        if remove_first and G:
            keep[np.argsort(d[i], kind="stable")[0]] = False
        di, ri = d[i][keep], rel[i][keep]
        total = int(ri.sum())
        for t, r in enumerate(radii):
            inside = di <= r
            retrieved[i, t] = int(inside.sum())
            hits[i, t] = int((inside & ri).sum())
            P[i, t] = hits[i, t] / retrieved[i, t] if retrieved[i, t] else 0.0
            R[i, t] = hits[i, t] / total if total else 0.0
    mean = lambda a: a.mean(axis=0) if Qn else np.zeros(len(radii))
    return dict(retrieved=retrieved, hits=hits, precisions=mean(P), recalls=mean(R), retrieved_mean=mean(retrieved.astype(np.float64)),
                empty=mean((retrieved == 0).astype(np.float64)))


def clustered(labels, centres, nbit, seed, flip=0.1):
    """packed uint64 codes: each row its class centre with every bit flipped with probability `flip` -- deep distance buckets"""
    rng = np.random.default_rng(seed)
    bits = centres[labels] ^ (rng.random((len(labels), nbit)) < flip).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8")
