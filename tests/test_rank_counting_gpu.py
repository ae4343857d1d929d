"""GPU: the one rank-counting pipeline (`retrieval._evaluate_by_rank_counting`: collect, sort, count, AP) gives one answer under every
distance where the mathematics says it must.  On +-1 codes every weight of the asymmetric distance is 2^P - 1, so D = (2^P - 1) H; at
margin 0.5 no entry is unsure, so K = 2 H; dot gives 2 H - n, squared Euclidean 4 H, and at n = 64 cosine gives 2 H / n, exact in fp32
(1 / sqrt(120) is no power of two, so at n = 120 fp32 rounding may split cosine ties: left out there).  Hence every ranking, and every
tie, is the Hamming ranking, and every evaluation must equal the brute force of tests/asymmetric_eval_ref.py on the numpy Hamming matrix
bit for bit -- with lists searched in LDS and, at list_cap = 4, in global memory."""
import numpy as np
import pytest
import torch

import asymmetric_eval_ref as aref

pytestmark = pytest.mark.gpu

QN, G, C = 37, 771, 7     # three query tiles of 16, the last with 5; at seg_rows = 256 three whole segments and a 3-row tail
SEG = 256
KS = (1, 5, 10)
_problems = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _problem(n):
    """+-1 codes (class centres with 10 % of the signs flipped), labels, and the brute-force integers per (remove_first, R); built once"""
    if n not in _problems:
        rng = np.random.default_rng(1000 + n)
        centres = np.where(rng.random((C, n)) < 0.5, -1.0, 1.0)
        gl, ql = rng.integers(0, C, G), rng.integers(0, C, QN)

        def codes(labels):
            flip = rng.random((labels.size, n)) < 0.1
            return (centres[labels] * np.where(flip, -1.0, 1.0)).astype(np.float32)
        xq, xg = codes(ql), codes(gl)
        ql[3] = C                                                                   # a class the gallery does not hold
        H = (n - xq.astype(np.int64) @ xg.astype(np.int64).T) // 2
        assert np.array_equal(H, (xq[:, None, :] != xg[None, :, :]).sum(-1))
        assert int((np.diff(np.sort(H, axis=1), axis=1) == 0).sum()) > 1000         # the ties are what the rankings must agree on
        rel = aref.relevance(ql, gl)
        want = {(rf, R): aref.evaluate(H, rel, [R] + list(KS), rf) for rf in (False, True) for R in (-1, 50)}
        assert all(w[2][3] == 0 for w in want.values())                             # query 3 has no relevant row
        _problems[n] = xq, xg, ql, gl, want
    return _problems[n]


def _check(out, want, where):
    S, nrel, total = want                                                           # limits were [R] + KS
    assert np.array_equal(out["S"].cpu().numpy().view(np.uint64), S[0]), where
    assert np.array_equal(out["nrel"].cpu().numpy(), nrel[0]), where
    assert np.array_equal(out["total"].cpu().numpy(), total) and int(out["total"][3]) == 0, where
    assert np.array_equal(out["hits"].cpu().numpy(), nrel[1:].T), where


@pytest.mark.parametrize("list_cap", [None, 4])
@pytest.mark.parametrize("n", [64, 120])
def test_every_ranking_is_the_hamming_ranking_on_sign_codes(dev, n, list_cap):
    from concepthash_amd import retrieval as rt
    xq, xg, ql, gl, want = _problem(n)
    q, g = torch.from_numpy(xq).to(dev), torch.from_numpy(xg).to(dev)
    q_lab, g_lab = torch.from_numpy(ql).to(dev), torch.from_numpy(gl).to(dev)
    packed = rt.pack_sign(g)
    q3, g3 = rt.pack_ternary(q, 0.5), rt.pack_ternary(g, 0.5)
    for (rf, R), w in want.items():
        how = dict(R=R, ks=KS, remove_first=rf, seg_rows=SEG, list_cap=list_cap)
        for bits in (4, 8):
            _check(rt.evaluate_weighted(q, packed, q_lab, g_lab, bits=bits, **how), w, ("weighted", bits, rf, R))
        _check(rt.evaluate_ternary(q3, g3, n, q_lab, g_lab, **how), w, ("ternary", rf, R))
        for metric in ("dot", "euclidean") + (("cosine",) if n == 64 else ()):
            _check(rt.evaluate_dense(q, g, q_lab, g_lab, metric, **how), w, (metric, rf, R))
