"""fp64 numpy reference of the reduction ("reduction"; csrc/pca.hip), the bounds the GPU tests hold it to with
their derivations, and the input constructions the CPU and GPU tests share.  numpy and torch only.

Block-structured matrices are compact throughout: A [n, t], row b s + l = A_b[l, :] (s = n / blocks columns in, t out per block).

Bounds (u = 2^-24, gamma_L = L u / (1 - L u), Higham's constant for L roundings):
  * y = fl32(x - shift) is ONE rounding the kernels and this reference both make (numpy's float32 subtraction), so the reference's
    moments are those of the SAME y: the subtraction puts no term into a bound.
  * gram: inside a segment an entry is the chain acc = fmaf(y_a, y_c, acc) from 0 over c <= L = min(rows, seg_rows) rows: c roundings,
    |chain - exact| <= gamma_c sum |y_a y_c| over the segment's rows.  The segments' partials (each a float) are added in fp64: nseg - 1
    roundings of at most 2^-53 relative each.  The bound the tests hold the kernels to counts that combine as 2^-50 relative to
    sum_i |y_a y_c|: rigorous up to 9 segments ((nseg - 1) 2^-53 (1 + gamma)); beyond that it relies on the roundings of the combine not
    all pointing one way (their worst case at the tests' 4,097 segments is 2^-41, still 2^-17 of gamma_1), and the GPU test prints how
    much of its bound the largest error uses.
    So |gram - ref| <= (gamma_L + 2^-50) sum_i |y_a y_c|.
  * sum: a fixed tree of plain fp32 adds over the segment's rows, at most L - 1 adds on any path: |sum - exact| <= gamma_L sum_i |y|,
    and the same fp64 combine.
  * projection: the chain of s fmaf from 0: |out - exact| <= gamma_s sum_l |y_l| |A_lj|.
  * fit (`fit_epsilon`): the fit diagonalises C' = (gram' - sum' sum'^T / N) / (N - 1) made of the GPU's moments, the test scores it on
    C = the same expression in exact arithmetic (the fp64 covariance of y).  E = C' - C has
    |E_ac| <= (Bg_ac + (|s_a| Bs_c + Bs_a |s_c| + Bs_a Bs_c) / N) / (N - 1) with Bg, Bs the moment bounds above and s the exact sums, so
    ||E||_2 <= ||E||_F <= eps := the Frobenius norm of that matrix.  For A with orthonormal columns spanning the top-t eigenspace of
    C' (any rotation of the eigenvectors: a rotation keeps the trace):
        tr(A^T C A) = tr(A^T C' A) - tr(A^T E A) >= sum_{j<=t} lambda_j(C') - t eps        (|tr(A^T E A)| <= t ||E||_2)
                    >= sum_{j<=t} (lambda_j(C) - eps) - t eps = sum_{j<=t} lambda_j(C) - 2 t eps      (Weyl: |lambda_j(C') - lambda_j(C)| <= ||E||_2).
    What is not exact about A -- fp64 eigh, the fp64 product P R, the rounding of A to fp32, R's orthogonality to 1e-5 -- is covered by
    the test's 1e-5 tr(C) term.
"""
import numpy as np

import itq_ref as ir

U = 2.0 ** -24


def gamma(L):
    return L * U / (1.0 - L * U)


def shifted(X, shift=None):
    """y = fl32(x - shift) as fp64 values (y = x without a shift)"""
    X = np.asarray(X, np.float32)
    return (X if shift is None else X - np.asarray(shift, np.float32)[None, :]).astype(np.float64)


def block_gram(Y, s):
    """[rows, n] fp64 -> [n, s]: row b s + a = sum_i y[i, b s + a] y[i, b s : (b + 1) s]"""
    n = Y.shape[1]
    return np.concatenate([Y[:, b * s:(b + 1) * s].T @ Y[:, b * s:(b + 1) * s] for b in range(n // s)]) if n else np.zeros((0, s))


def moments(X, s, shift=None):
    """-> (sum [n], gram [n, s]) of y = fl32(x - shift), in fp64"""
    Y = shifted(X, shift)
    return Y.sum(0), block_gram(Y, s)


def moment_bounds(X, s, L, shift=None):
    """-> (bound of sum [n], bound of gram [n, s]) for fp32 chains of at most L rows and the fp64 combine (module docstring)"""
    Y = np.abs(shifted(X, shift))
    g = gamma(L) + 2.0 ** -50
    return g * Y.sum(0), g * block_gram(Y, s)


def default_seg_rows(rows):
    """the library's rule where seg_rows is left open: about 1,024 segments, 64 .. 4,096 rows, a multiple of 64"""
    return int(max(64, min(4096, -(-(-(-max(rows, 1) // 1024)) // 64) * 64)))


def covariance(total, gram, N):
    """per block C_b = (gram_b - sum_b sum_b^T / N) / (N - 1) -> [blocks, s, s]"""
    n, s = gram.shape
    sb = total.reshape(n // s, s)
    return (gram.reshape(n // s, s, s) - sb[:, :, None] * sb[:, None, :] / N) / (N - 1)


def signed(P):
    """each column signed so that its entry of largest magnitude is positive, the lowest index among equals"""
    lead = np.abs(P).argmax(0)
    return P * np.where(P[lead, np.arange(P.shape[1])] < 0, -1.0, 1.0)[None, :]


def components(C, t):
    """C [blocks, s, s] -> (P [blocks, s, t], eigenvalues [blocks, s] descending), numpy.linalg.eigh and the sign convention"""
    Ps, lams = [], []
    for Cb in C:
        lam, vec = np.linalg.eigh(Cb)
        lams.append(lam[::-1])
        Ps.append(signed(vec[:, ::-1][:, :t]))
    return np.stack(Ps), np.stack(lams)


def project(X, mean, Ac, s):
    """out [rows, blocks t] fp64, A compact [n, t], blocks of s rows: for output j of block b, acc = 0; for l = 0 .. s-1 in this order:
    acc += fl32(x[:, b s + l] - mean[b s + l]) A_b[l, j]"""
    Y, Ac = shifted(X, mean), np.asarray(Ac, np.float64)
    n, t = Ac.shape
    out = np.zeros((Y.shape[0], n // s * t))
    for b in range(n // s):
        for l in range(s):
            out[:, b * t:(b + 1) * t] += Y[:, b * s + l, None] * Ac[b * s + l][None, :]
    return out


def project_bound(X, mean, Ac, s):
    """gamma_s sum_l |y_l| |A_lj| per output"""
    n, t = Ac.shape
    Y, A = np.abs(shifted(X, mean)), np.abs(np.asarray(Ac, np.float64))
    return gamma(s) * np.concatenate([Y[:, b * s:(b + 1) * s] @ A[b * s:(b + 1) * s] for b in range(n // s)], axis=1)


def fit(X, bits, blocks, method="pca-itq", iters=50):
    """retrieval.fit_reduction in fp64: mean = fp32(sum / N); C of y = fl32(x - mean); P; V = the projection chain, stored as fp32;
    pca-itq: the reference ITQ fit on V (itq_ref.fit), A = fp32(P R).  -> dict(mean fp32 [n], A compact fp32 [n, t], P, eigenvalues,
    C, explained_share, iters_run)"""
    X = np.asarray(X, np.float32)
    N, n = X.shape
    s, t = n // blocks, bits // blocks
    mean = (X.astype(np.float64).sum(0) / N).astype(np.float32)
    total, gram = moments(X, s, mean)
    C = covariance(total, gram, N)
    P, lam = components(C, t)
    Pc = P.reshape(n, t).astype(np.float32)
    trace = float(np.trace(C, axis1=1, axis2=2).sum())
    out = dict(mean=mean, P=P, eigenvalues=lam, C=C, explained_share=float(lam[:, :t].sum()) / trace if trace > 0 else 0.0, iters_run=0, A=Pc)
    if method == "pca-itq":
        V = project(X, mean, Pc, s).astype(np.float32)
        rot = ir.fit(V, t, iters=iters)
        R = rot["R"].reshape(blocks, t, t)
        out.update(A=(P @ R).reshape(n, t).astype(np.float32), iters_run=rot["iters_run"])
    return out


def fit_epsilon(X, mean, s, L):
    """eps of the module docstring, per block: -> [blocks]"""
    N, n = np.asarray(X).shape
    total, _ = moments(X, s, mean)
    Bs, Bg = moment_bounds(X, s, L, mean)
    blocks = n // s
    sa, ba = np.abs(total).reshape(blocks, s), Bs.reshape(blocks, s)
    E = (Bg.reshape(blocks, s, s) + (sa[:, :, None] * ba[:, None, :] + ba[:, :, None] * sa[:, None, :] + ba[:, :, None] * ba[:, None, :]) / N) / (N - 1)
    return np.sqrt((E * E).sum((1, 2)))


def truncated_columns(n, bits, blocks):
    """the first bits / blocks columns of every block"""
    s, t = n // blocks, bits // blocks
    return (np.arange(blocks)[:, None] * s + np.arange(t)[None, :]).reshape(-1)


def hamming_map(q, g, q_lab, g_lab):
    """mAP@all of the Hamming ranking of sign codes (bit = value > 0), rows ordered by ascending (distance, index)"""
    Bq, Bg = np.asarray(q) > 0, np.asarray(g) > 0
    aps = []
    for i in range(Bq.shape[0]):
        order = np.argsort((Bq[i][None, :] != Bg).sum(1), kind="stable")
        rel = (g_lab[order] == q_lab[i]).astype(np.float64)
        aps.append(float((np.cumsum(rel) / np.arange(1, len(rel) + 1) * rel).sum() / rel.sum()) if rel.sum() else 0.0)
    return float(np.mean(aps))


# ---- input constructions -----------------------------------------------------------------------------------------------------------
def grid_case(rows, n, seed=0, with_shift=True):
    """entries and shift: multiples of 1/16 in [-2, 2].  Then |y| <= 4, a product y_a y_c is a multiple of 2^-8 of at most 16, and a
    chain of at most 4,096 of them stays below 2^24 units of 2^-8: every fp32 partial sum is exact, in any order and segmentation.
    -> (X fp32 [rows, n], shift fp32 [n] or None)"""
    rng = np.random.default_rng(seed)
    X = (rng.integers(-32, 33, size=(rows, n)) / 16.0).astype(np.float32)
    shift = (rng.integers(-32, 33, size=n) / 16.0).astype(np.float32) if with_shift else None
    return X, shift


def grid_matrix(n, t, seed=0):
    """A compact [n, t]: multiples of 1/16 in [-1, 1] (a chain of at most 256 products |y a| <= 4, multiples of 2^-8, is exact in fp32)"""
    return (np.random.default_rng(seed).integers(-16, 17, size=(n, t)) / 16.0).astype(np.float32)


def gaussian_case(rows, n, seed=0, offset=3.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, n)) + offset).astype(np.float32)


def planted_case(sigma, seed=0, classes=20, per_class=40, blocks=4, latent=8, queries=150):
    """classes x per_class rows of `blocks` blocks of 2 `latent` dimensions each: `latent` dimensions of +-1 class centres plus N(0, sigma^2) beside
    `latent` dimensions of N(0, 0.15^2), the block through a random orthogonal matrix, plus 0.7.  `queries` rows, drawn at random, are
    the queries, the others the database.  -> (db fp32, db labels, q fp32, q labels)"""
    rng = np.random.default_rng(seed)
    s = 2 * latent
    lab = np.repeat(np.arange(classes), per_class)
    cols = []
    for _ in range(blocks):
        centres = np.where(rng.random((classes, latent)) < 0.5, -1.0, 1.0)
        Z = np.concatenate([centres[lab] + sigma * rng.standard_normal((len(lab), latent)), 0.15 * rng.standard_normal((len(lab), latent))], axis=1)
        Q = np.linalg.qr(rng.standard_normal((s, s)))[0]
        cols.append(Z @ Q + 0.7)
    X = np.concatenate(cols, axis=1).astype(np.float32)
    perm = rng.permutation(len(lab))
    qi, gi = np.sort(perm[:queries]), np.sort(perm[queries:])
    return X[gi], lab[gi], X[qi], lab[qi]


def planted_maps(sigma, seed=0, bits=32, blocks=4):
    """mAP@all of the full / truncated / PCA / PCA-ITQ sign codes of `planted_case`, all in fp64: the plain codes are x - the database
    mean (the zero-mean shift of the evaluator), truncated their first bits / blocks columns per block; the fits are made on the
    database"""
    g, gl, q, ql = planted_case(sigma, seed)
    n = g.shape[1]
    s = n // blocks
    mean = g.astype(np.float64).mean(0).astype(np.float32)
    g0, q0 = shifted(g, mean), shifted(q, mean)
    cols = truncated_columns(n, bits, blocks)
    out = dict(full=hamming_map(q0, g0, ql, gl), truncated=hamming_map(q0[:, cols], g0[:, cols], ql, gl))
    for method in ("pca", "pca-itq"):
        f = fit(g, bits, blocks, method)
        out[method] = hamming_map(project(q, f["mean"], f["A"], s), project(g, f["mean"], f["A"], s), ql, gl)
    return out


if __name__ == "__main__":
    for sigma in (0.7, 0.9, 1.1):
        print(sigma, {k: round(v, 3) for k, v in planted_maps(sigma).items()})
