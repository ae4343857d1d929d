"""CPU: the definition of the tie bracket -- the closed form of tests/tie_bracket_ref.py against a brute force
over every order inside the distance buckets, against the stable ranking of oracle/hamming_oracle.py, and the two mean conventions."""
import numpy as np
import pytest

import tie_bracket_ref as tb


def _tiny_problems(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        nbuckets = int(rng.integers(1, 4))
        ns = [int(rng.integers(1, 5)) for _ in range(nbuckets)]
        if sum(ns) > 8:
            continue
        out.append([(n, int(rng.integers(0, n + 1))) for n in ns])
    return out


def test_cut_bucket_hand_example():
    """Stable prefix `rel, irr`, then a bucket {rel, irr}, R = 3: relevant-first gives (1 + 2/3) / 2 = 0.833, irrelevant-first gives
    1 / 1 = 1 -- inside the bucket a limit cuts, "relevant rows first" is NOT the maximum."""
    buckets = [(1, 1), (1, 0), (2, 1)]
    lo, nlo, hi, nhi = tb.bracket_one(buckets, 3, exact=False)
    assert hi / nhi == 1.0 and nhi == 1
    assert abs(lo / nlo - (1 + 2 / 3) / 2) < 1e-15 and nlo == 2
    assert tb.brute_force(buckets, 3) == (pytest.approx((1 + 2 / 3) / 2, abs=1e-15), 1.0)
    S_lo, n_lo, S_hi, n_hi = tb.bracket_one(buckets, 3, exact=True)
    assert (S_hi, n_hi) == (1 << 32, 1) and (S_lo, n_lo) == ((1 << 32) + (2 << 32) // 3, 2)


@pytest.mark.parametrize("remove_first", [False, True])
def test_closed_form_equals_brute_force(remove_first):
    cases = 0
    for buckets in _tiny_problems(300, seed=11):
        G = sum(n for n, _ in buckets)
        for R in list(range(1, G + 1)) + [-1]:
            lo, nlo, hi, nhi = tb.bracket_one(buckets, R, remove_first, exact=False)
            blo, bhi = tb.brute_force(buckets, R, remove_first)
            assert abs(tb.ap_value(lo, nlo, False) - blo) < 1e-12, (buckets, R, remove_first)
            assert abs(tb.ap_value(hi, nhi, False) - bhi) < 1e-12, (buckets, R, remove_first)
            # the integers describe the same two orders: 2^-32 fixed point, one floor per relevant row
            S_lo, n_lo, S_hi, n_hi = tb.bracket_one(buckets, R, remove_first, exact=True)
            assert abs(tb.ap_value(S_lo, n_lo) - blo) < 8 * 2.0 ** -32 and abs(tb.ap_value(S_hi, n_hi) - bhi) < 8 * 2.0 ** -32
            cases += 1
    assert cases > 1000


@pytest.mark.parametrize("remove_first", [False, True])
def test_hits_bracket_equals_brute_force(remove_first):
    for buckets in _tiny_problems(120, seed=12):
        G = sum(n for n, _ in buckets)
        for k in range(1, G + 1):
            lo, hi, rlo, rhi = tb.hits_extremes(buckets, k, remove_first)
            blo, bhi, brlo, brhi = tb.brute_force(buckets, -1, remove_first, k=k)
            assert (lo, hi) == (blo, bhi), (buckets, k, remove_first)
            assert abs(rlo - brlo) < 1e-15 and abs(rhi - brhi) < 1e-15, (buckets, k, remove_first)


def _tied_codes(rows, bits, seed, nclass):
    """packed 64-bit codes that differ in `bits` low bits only: at most bits + 1 distinct distances -> deep buckets"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << bits, size=(rows, 1), dtype=np.uint64), rng.integers(0, nclass, size=rows).astype(np.int32)


@pytest.mark.parametrize("remove_first", [False, True])
@pytest.mark.parametrize("R", [-1, 1, 7, 40, 299, 300])
def test_stable_ap_lies_inside_the_bracket(R, remove_first):
    from oracle import hamming_oracle as ho
    q, ql = _tied_codes(23, 3, 1, 4)
    g, gl = _tied_codes(300, 3, 2, 4)
    ref = ho.mean_ap(q, g, ql, gl, R=R, ks=(1, 5, 10), remove_first=remove_first, want_hist=True)
    counts = tb.counts_from_codes(q, g, ql, gl)
    assert np.array_equal(counts, ref["hist"])
    S_lo, n_lo, S_hi, n_hi = tb.bracket_from_counts(counts, [R], remove_first)
    lo, hi = tb.ap_from_fixed(S_lo[0], n_lo[0]), tb.ap_from_fixed(S_hi[0], n_hi[0])
    assert (lo <= ref["ap_fixed"]).all() and (ref["ap_fixed"] <= hi).all()
    assert (lo < hi).any()                                 # 300 rows on four distances: the order inside the buckets matters
    for t, k in enumerate((1, 5, 10)):
        for qi in range(len(q)):
            hlo, hhi, _, _ = tb.hits_extremes(counts[qi], k, remove_first)
            assert hlo <= ref["hits"][qi, t] <= hhi


@pytest.mark.parametrize("R", [-1, 3, 20])
def test_bracket_collapses_without_ties_and_in_pure_buckets(R):
    from oracle import hamming_oracle as ho
    # every bucket holds one row: gallery row j has its j low bits set, the query is 0 -> distance j
    g = np.array([[(1 << j) - 1] for j in range(40)], dtype=np.uint64)
    gl = (np.arange(40) % 3).astype(np.int32)
    q = np.zeros((3, 1), dtype=np.uint64)
    ql = np.arange(3, dtype=np.int32)
    # every bucket all-relevant or all-irrelevant: the class decides the distance
    g2 = np.array([[(1 << (1 + 5 * (j % 4))) - 1] for j in range(60)], dtype=np.uint64)
    gl2 = (np.arange(60) % 4).astype(np.int32)
    for codes, labels in ((g, gl), (g2, gl2)):
        ref = ho.mean_ap(q, codes, ql, labels, R=R, ks=())
        S_lo, n_lo, S_hi, n_hi = tb.bracket_from_counts(tb.counts_from_codes(q, codes, ql, labels), [R])
        assert np.array_equal(S_lo[0], ref["S"]) and np.array_equal(S_hi[0], ref["S"])
        assert np.array_equal(n_lo[0], ref["nrel"]) and np.array_equal(n_hi[0], ref["nrel"])


def test_the_two_mean_conventions():
    """Three queries at R = 2.  Query 0: one bucket {irr, irr, rel}: no relevant row inside R under the pessimistic order (AP 0, nrel 0),
    one under the optimistic (AP 1).  Query 1: relevant at rank 1 whatever the order.  Query 2: no relevant row at all.
    skip_queries_without_relevant=False: every query counts.  True: a query counts in mAP_high iff its optimistic order has a relevant
    row inside R, in mAP_low iff its pessimistic order has one."""
    counts = np.zeros((3, 65, 2), dtype=np.uint32)
    counts[0, 4] = (3, 1)
    counts[1, 0] = (1, 1)
    counts[1, 9] = (5, 0)
    counts[2, 7] = (4, 0)
    S_lo, n_lo, S_hi, n_hi = tb.bracket_from_counts(counts, [2])
    lo, hi = tb.ap_from_fixed(S_lo[0], n_lo[0]), tb.ap_from_fixed(S_hi[0], n_hi[0])
    assert lo.tolist() == [0.0, 1.0, 0.0] and hi.tolist() == [1.0, 1.0, 0.0]
    assert n_lo[0].tolist() == [0, 1, 0] and n_hi[0].tolist() == [1, 1, 0]
    assert lo.mean() == pytest.approx(1 / 3) and hi.mean() == pytest.approx(2 / 3)          # every query in the mean
    assert lo[n_lo[0] > 0].mean() == 1.0 and hi[n_hi[0] > 0].mean() == 1.0                  # queries without a relevant row left out
    # the project's own summarize() applies the same two conventions to the bracket integers (host arithmetic, no kernel)
    import torch
    from concepthash_amd import retrieval as rt
    t = lambda a, dt: torch.from_numpy(a.astype(dt))
    total = torch.zeros(3, dtype=torch.int32)
    for skip, want_lo, want_hi in ((False, 1 / 3, 2 / 3), (True, 1.0, 1.0)):
        m_lo = rt.summarize(t(S_lo, np.int64), t(n_lo, np.int32), total, [0], [2], [], skip)["mAPs"][0]
        m_hi = rt.summarize(t(S_hi, np.int64), t(n_hi, np.int32), total, [0], [2], [], skip)["mAPs"][0]
        assert m_lo == pytest.approx(want_lo) and m_hi == pytest.approx(want_hi)


def test_the_entry_point_is_declared_and_validates_its_arguments_on_the_host():
    """no GPU: the symbol is bound, and bad limits / sizes / alignment are refused before anything is launched"""
    import ctypes
    from concepthash_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert "ch_hamming_tie_bracket" in _lib.SIGNATURES
    lims = (ctypes.c_int64 * 2)(5, 3)
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its argument checks
    assert lib.ch_hamming_tie_bracket(fake, 4, 65, lims, 0, 0, fake, fake, fake, fake, None) != 0 and b"nlimits" in lib.ch_last_error()
    assert lib.ch_hamming_tie_bracket(fake, 4, 300, lims, 2, 0, fake, fake, fake, fake, None) != 0 and b"nb" in lib.ch_last_error()
    assert lib.ch_hamming_tie_bracket(fake, 4, 65, lims, 2, 0, fake, fake, fake, fake, None) != 0 and b"ascend" in lib.ch_last_error()
    lims = (ctypes.c_int64 * 2)(3, -1)
    assert lib.ch_hamming_tie_bracket(ctypes.c_void_p(4100), 4, 65, lims, 2, 0, fake, fake, fake, fake, None) != 0
    assert b"aligned" in lib.ch_last_error()
    assert lib.ch_hamming_tie_bracket(None, 0, 65, lims, 2, 0, None, None, None, None, None) == 0      # no query: nothing to do
