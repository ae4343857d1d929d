"""fp64 numpy reference of the learned rotation ("learned rotation"; csrc/itq.hip) and the input constructions
the CPU and GPU tests share.  R is compact throughout: [n, s], row b s + l = R_b[l, :].
"""
import numpy as np


def chain(V, Rc):
    """z [G, n] fp64: for output j of block b, acc = 0; for l = 0 .. s-1: acc += V[:, b s + l] R_b[l, j - b s], in this order"""
    V, Rc = np.asarray(V, np.float64), np.asarray(Rc, np.float64)
    n, s = Rc.shape
    z = np.zeros((V.shape[0], n))
    for b in range(n // s):
        for l in range(s):
            z[:, b * s:(b + 1) * s] += V[:, b * s + l, None] * Rc[b * s + l][None, :]
    return z


def sign(z):
    """+1 where z > 0, else -1: an exact zero is a 0 bit"""
    return np.where(z > 0, 1.0, -1.0)


def stats(z):
    """(L1 = sum |z|, cosine sum = sum_i |z_i|_1 / (sqrt(n) |z_i|_2) with a zero row adding 0, qerr = 1 - cosine sum / G)"""
    l1 = np.abs(z).sum(1)
    l2 = np.sqrt((z * z).sum(1))
    cos = np.where(l2 > 0, l1 / (np.sqrt(z.shape[1]) * np.where(l2 > 0, l2, 1.0)), 0.0)
    return float(l1.sum()), float(cos.sum()), float(1.0 - cos.sum() / max(z.shape[0], 1))


def step(V, Rc):
    """-> (M [n, s]: row j = sum_i B_ij V[i, block of j], L1, cosine sum, qerr, z)"""
    V = np.asarray(V, np.float64)
    n, s = Rc.shape
    z = chain(V, Rc)
    B = sign(z)
    M = np.concatenate([B[:, b * s:(b + 1) * s].T @ V[:, b * s:(b + 1) * s] for b in range(n // s)])
    return (M,) + stats(z) + (z,)


def procrustes(M):
    """M_b = U S W^T -> R_b = W U^T, block by block"""
    n, s = M.shape
    out = np.empty_like(M)
    for b in range(n // s):
        U, _, Wh = np.linalg.svd(M[b * s:(b + 1) * s])
        out[b * s:(b + 1) * s] = (U @ Wh).T
    return out


def identity(n, s):
    return np.tile(np.eye(s), (n // s, 1))


def fit(V, s, iters=50, tol=1e-6, store=np.float32):
    """The fit of retrieval.fit_rotation: pass t scores R_t, R_0 = I, R stored as fp32 between passes -> dict(R compact fp64 values of
    the stored rotation, iters_run, l1, qerr_before, qerr_after)"""
    n = V.shape[1]
    R = identity(n, s)
    l1s, best, before = [], None, None
    for t in range(iters + 1):
        M, l1, _, qerr, _ = step(V, R)
        l1s.append(l1)
        before = qerr if t == 0 else before
        if best is None or l1 > best[0]:
            best = (l1, R, t, qerr)
        if t == iters or (t >= 1 and l1 - l1s[-2] <= tol * l1s[-2]):
            break
        R = procrustes(M).astype(store).astype(np.float64)
    return dict(R=best[1], iters_run=best[2], l1=l1s, qerr_before=before, qerr_after=best[3])


def full(Rc):
    n, s = Rc.shape
    out = np.zeros((n, n), Rc.dtype)
    for b in range(n // s):
        out[b * s:(b + 1) * s, b * s:(b + 1) * s] = Rc[b * s:(b + 1) * s]
    return out


# ---- input constructions -----------------------------------------------------------------------------------------------------------
def hadamard(s):
    H = np.ones((1, 1))
    while H.shape[0] < s:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == s, "s must be a power of two"
    return H


def exact_case(G, n, s, seed=0):
    """R_b = H_s / sqrt(s) (exact in fp32 for s a power of 4) and V = odd multiples of 2^-8 in [-2, 2]: every partial sum of z and of M is
    exact in fp32 in any order.  -> (V fp32 [G, n], R compact fp32 [n, s])"""
    assert s in (4, 16, 64, 256)
    rng = np.random.default_rng(seed)
    V = ((2 * rng.integers(-256, 256, size=(G, n)) + 1) / 256.0).astype(np.float32)
    V[: min(G, 4), :] = (np.array([1, -1, 3, -3])[: min(G, 4), None] / 256.0)   # constant rows: their z is an exact zero wherever H has a zero row sum
    R = np.tile(hadamard(s) / np.sqrt(s), (n // s, 1)).astype(np.float32)
    return V, R


def qr_rotation(n, s, rng):
    return np.concatenate([np.linalg.qr(rng.standard_normal((s, s)))[0] for _ in range(n // s)]).astype(np.float32)


def tau(V, R):
    """the margin under which an fp32 chain could decide a sign differently: 4 n 2^-24 max_i |v_i|_1 max |R|"""
    return 4 * V.shape[1] * 2.0 ** -24 * np.abs(V.astype(np.float64)).sum(1).max() * np.abs(R).max()


def general_case(G, n, s, seed=0):
    """Gaussian V, R from a QR per block; rows are drawn until G of them have min_j |z_ij| >= tau under the fp64 chain.
    -> (V fp32 [G, n], R compact fp32 [n, s], tau)"""
    rng = np.random.default_rng(seed)
    R = qr_rotation(n, s, rng)
    kept, t = [], 0.0
    while sum(len(k) for k in kept) < G:
        V = rng.standard_normal((2 * G, n)).astype(np.float32)
        t = max(t, tau(V, R))
        kept.append(V)
        allv = np.concatenate(kept)
        ok = np.abs(chain(allv, R)).min(1) >= t
        kept = [allv[ok]]
    V = kept[0][:G]
    assert np.abs(chain(V, R)).min() >= tau(V, R)
    return V, R, tau(V, R)


def givens_rotation(s, degrees=30.0):
    c, sn = np.cos(np.deg2rad(degrees)), np.sin(np.deg2rad(degrees))
    Q = np.eye(s)
    for p in range(0, s - 1, 2):
        Q[p:p + 2, p:p + 2] = [[c, -sn], [sn, c]]
    return Q


def planted_case(G, n, s, seed=0):
    """X = B0 * a, a in (0.5, 1.5), V = X Q0^T with Q0 made of 30-degree Givens rotations of the dimension pairs inside each block: the
    rotation Q0 takes V back to X, whose quantisation error is the floor.  -> V fp32 [G, n]"""
    rng = np.random.default_rng(seed)
    X = np.where(rng.random((G, n)) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 1.5, size=(G, n))
    Q = givens_rotation(s)
    V = np.concatenate([X[:, b * s:(b + 1) * s] @ Q.T for b in range(n // s)], axis=1)
    return V.astype(np.float32)


def clustered_case(G, n, seed=0, classes=20, noise=0.6):
    """class centres in {-1, +1}^n rotated by one random orthogonal matrix, plus Gaussian noise -> (V fp32 [G, n], labels int64 [G])"""
    rng = np.random.default_rng(seed)
    centres = np.where(rng.random((classes, n)) < 0.5, -1.0, 1.0)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lab = rng.integers(0, classes, size=G)
    V = centres[lab] @ Q + noise * rng.standard_normal((G, n))
    return V.astype(np.float32), lab.astype(np.int64)
