"""No GPU: the tie expectation -- the Fraction closed form of tests/tie_expected_ref.py against the enumeration
of every tie order, against the tie bracket and the stable order; the float64 form of the kernel's arithmetic against its derived bound;
and the refusals and the evaluator class, through the Python layers that need no GPU."""
import json
import os
import random
import sys
from fractions import Fraction

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tie_bracket_ref as tb   # noqa: E402
import tie_expected_ref as te  # noqa: E402

KS = (1, 2, 3, 5)
BRUTE_CAP = 300      # tie orders (distinct relevance patterns) enumerated per problem at the most


def tiny_problems(count, seed):
    """random problems of <= 4 buckets of <= 4 rows whose enumeration stays under BRUTE_CAP orders"""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        b = []
        for _ in range(rng.randint(1, 4)):
            n = rng.randint(0, 4)
            b.append((n, rng.randint(0, n)))
        if te.brute_force_size(b) <= BRUTE_CAP:
            out.append(b)
    return out


def test_closed_form_equals_every_tie_order_exactly():
    checked = 0
    for b in tiny_problems(300, seed=1):
        G = sum(n for n, _ in b)
        Rs = list(range(0, G + 2))
        for rf in (False, True):
            ap, hits, rec = te.brute_force(b, Rs, KS, rf)
            for R in Rs:
                got = te.expected_one(b, R, KS, rf)
                assert isinstance(got[0], Fraction) and got[0] == ap[R], (b, R, rf, got[0], ap[R])
                assert got[1] == [hits[k] for k in KS] and got[2] == [rec[k] for k in KS], (b, rf)
                checked += 1
    assert checked > 3000


def test_expectation_lies_inside_the_bracket_and_fixed_point_agrees():
    fx = te.Fixed()
    for b in tiny_problems(120, seed=2):
        G = sum(n for n, _ in b)
        for rf in (False, True):
            for R in range(0, G + 2):
                e = te.expected_one(b, R, (), rf)[0]
                S_lo, n_lo, S_hi, n_hi = tb.bracket_one(b, R, rf, exact=False)
                lo, hi = tb.ap_value(S_lo, n_lo, False), tb.ap_value(S_hi, n_hi, False)
                assert lo - 1e-15 <= float(e) <= hi + 1e-15, (b, R, rf, lo, float(e), hi)
                assert abs(fx.to_float(te.expected_one(b, R, (), rf, fx)[0]) - float(e)) <= 2.0 ** -52
            for k in KS:
                h_lo, h_hi, r_lo, r_hi = tb.hits_extremes(b, k, rf)
                _, h, rc = te.expected_one(b, None, (k,), rf)
                assert h_lo <= h[0] <= h_hi and r_lo - 1e-15 <= float(rc[0]) <= r_hi + 1e-15


def test_without_ties_the_expectation_is_the_stable_ap():
    rng = random.Random(3)
    for _ in range(50):
        flags = [rng.randint(0, 1) for _ in range(rng.randint(1, 12))]
        b = []
        for f in flags:
            b += [(1, f)] + [(0, 0)] * rng.randint(0, 2)
        for R in range(0, len(flags) + 2):
            lim = len(flags) if R <= 0 else min(R, len(flags))
            s, k = Fraction(0), 0
            for rank in range(1, lim + 1):
                if flags[rank - 1]:
                    k += 1
                    s += Fraction(k, rank)
            assert te.expected_one(b, R)[0] == (s / k if k else 0)
            assert te.expected_float64(b, [R] if R > 0 else [0])[0][0] == pytest.approx(float(s / k) if k else 0.0, abs=1e-15)


def deep_counts(seed, buckets=65, deepest=300):
    rng = random.Random(seed)
    out = []
    for _ in range(buckets):
        n = rng.randint(0, deepest) * (rng.random() < 0.5)
        out.append((n, int(n * rng.random())))
    return out


@pytest.mark.parametrize("remove_first", [False, True])
def test_float64_form_stays_inside_the_derived_bound(remove_first):
    """the kernel's arithmetic, in Python floats, on tiny problems (against Fractions) and on deep mixed buckets cut by 16 limits (against
    the 256-bit fixed point): every error under `error_bound`, and the bound itself far under the project's 1e-9"""
    worst = 0.0
    for b in tiny_problems(150, seed=4):
        G = sum(n for n, _ in b)
        lims = list(range(1, G + 2)) + [0]
        got_ap, got_h, got_r, _ = te.expected_float64(b, lims, KS, remove_first)
        for R, a in zip(lims, got_ap):
            err = abs(a - float(te.expected_one(b, R, (), remove_first)[0]))
            worst = max(worst, err)
            assert err <= te.error_bound(b, R, remove_first) < 1e-13
        _, h, rc = te.expected_one(b, None, KS, remove_first)
        for t, k in enumerate(KS):
            hb, rb = te.hits_bound(b, k, remove_first)
            assert abs(got_h[t] - float(h[t])) <= hb and abs(got_r[t] - float(rc[t])) <= rb
    fx = te.Fixed()
    lims = [1, 2, 3, 5, 8, 10, 20, 50, 64, 65, 100, 200, 500, 1000, 2999, 0]
    for seed in (5, 6):
        b = deep_counts(seed)
        got_ap, _, _, kept = te.expected_float64(b, lims, (), remove_first)
        assert kept > 64                                         # more than one trip of 64 weights: the early stop is exercised
        for R, a in zip(lims, got_ap):
            err = abs(a - fx.to_float(te.expected_one(b, R, (), remove_first, fx)[0]))
            worst = max(worst, err)
            assert err <= te.error_bound(b, R, remove_first) < 1e-9
    print(f"worst |float64 - exact| = {worst:.3g}")


def test_early_stop_keeps_o_sqrt_take_terms():
    """one bucket of 200,000 rows, half relevant, cut after 50,000: about 20 standard deviations (~ 112 each) are kept, not 50,000"""
    b = [(200000, 100000)]
    ap, _, _, kept = te.expected_float64(b, [50000])
    assert 64 <= kept <= 6000
    fx = te.Fixed()
    assert abs(ap[0] - fx.to_float(te.expected_one(b, 50000, (), False, fx)[0])) <= te.error_bound(b, 50000) < 1e-9


# ---- refusals: the Python layers in front of the GPU -----------------------------------------------------------------------------------
def _codes():
    g = torch.Generator().manual_seed(0)
    return torch.randn(30, 64, generator=g), torch.arange(30) % 3, torch.randn(6, 64, generator=g), torch.arange(6) % 3


def test_skip_queries_without_relevant_is_refused_with_the_reason():
    from concepthash_amd import retrieval as rt
    from utils import hashing
    db, dl, q, ql = _codes()
    with pytest.raises(ValueError, match="depends on the tie order"):
        hashing.calculate_mAP(db, dl, q, ql, -1, PRs=[1], tie_expected=True, skip_queries_without_relevant=True)
    packed = torch.zeros(4, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="depends on the tie order"):
        rt.evaluate(packed, packed, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), tie_expected=True,
                    skip_queries_without_relevant=True)
    with pytest.raises(ValueError, match="depends on the tie order"):
        rt.evaluate_gallery(rt.WholeGallery(packed, torch.zeros(4, dtype=torch.int32), rt), packed, torch.zeros(4, dtype=torch.int32),
                            tie_expected=True, skip_queries_without_relevant=True)


@pytest.mark.parametrize("rank,extra", [("asymmetric", {}), ("ternary", {"margin": 0.3}), ("cosine", {}), ("euclidean", {}), ("dot", {}),
                                        ("cosine", {"shortlist": 10})])
def test_other_ranks_refuse_the_expectation(rank, extra):
    from utils import hashing
    db, dl, q, ql = _codes()
    with pytest.raises(ValueError, match="tie expectation"):
        hashing.calculate_mAP(db, dl, q, ql, 5, PRs=[1], rank=rank, tie_expected=True, **extra)
    assert hashing.last_tie_expected is None


def test_entry_is_declared_bound_and_configured():
    from concepthash_amd import _lib
    import main_v2
    assert "ch_hamming_tie_expected" in _lib.SIGNATURES
    from concepthash_amd import build          # the error bound counts one rounding per operation: no contraction
    assert "hamming_tie_expected.hip" in build.SOURCES and build.EXTRA_FLAGS["hamming_tie_expected.hip"] == ["-ffp-contract=off"]
    header = open(os.path.join(ROOT, "include", "concepthash_hip.h")).read()
    assert "int ch_hamming_tie_expected(" in header
    assert "tie_expected" in main_v2.LOOP_KEYS
    for name in ("val.yaml", "train.yaml"):
        assert "tie_expected: False" in open(os.path.join(ROOT, "configs", name)).read()
    for mod in ("asymmetric_eval", "ternary_eval", "dense_eval", "rerank_eval"):
        assert '"tie_expected"' in open(os.path.join(ROOT, "experiments", mod + ".py")).read(), mod
    from experiments.text_eval import NOT_FOR_TEXT
    assert "tie_expected" in NOT_FOR_TEXT


@pytest.mark.parametrize("tie,concept", [(False, False), (True, False), (False, True), (True, True)])
def test_evaluator_records_the_expectation_beside_each_call(tmp_path, monkeypatch, tie, concept):
    """experiments.tie_expected_eval.TieExpectedEvaluation (under the concept evaluator that extends it) around a stub evaluator and a stub
    metric: every Hamming call asks for the expectation, its three lists land beside the call's own key, every concept's sub-code gets
    mAP_concept_expected, the bracket keeps working beside it, and the rebound names are restored."""
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.concept_eval import ConceptEvaluation
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, tie_bracket=False, tie_expected=False, PRs=None, **k):
        seen.append((tuple(db_codes.shape), bool(tie_bracket), bool(tie_expected)))
        m = float(db_codes.sum() + test_codes.sum())
        utils.hashing.last_tie_bracket = {"mAP_low": m - 1, "mAP_high": m + 1} if tie_bracket else None
        utils.hashing.last_tie_expected = {"mAP_expected": m + 0.5, "precisions_expected": [m + 0.25] * len(PRs),
                                           "recalls_expected": [m - 0.25] * len(PRs)} if tie_expected else None
        return m, [m] * len(PRs), [-m] * len(PRs)
    monkeypatch.setattr(utils.hashing, "calculate_mAP", metric)
    monkeypatch.setattr(base, "calculate_mAP", metric)
    db, te_codes = torch.arange(5 * 12, dtype=torch.float32).reshape(5, 12), -torch.arange(3 * 12, dtype=torch.float32).reshape(3, 12) / 7

    def evaluator_main(self):
        res = {}
        res["mAP"], res["recalls"], res["precisions"] = base.calculate_mAP(db, None, te_codes, None, -1, PRs=[1, 5], threshold=0)
        res["mAP_bin"], _, _ = base.calculate_mAP(db * 2, None, te_codes * 2, None, -1, PRs=[1, 5], threshold=0)
        self.results = res
        return res
    monkeypatch.setattr(base.RetrievalEvaluation, "main", evaluator_main)
    ev = ConceptEvaluation.__new__(ConceptEvaluation)
    ev.config = _wrap({"tie_expected": True, "concept_eval": concept, "compute_mAP": True, "exp": "validation", "tie_bracket": tie,
                       "sub_code_eval": False, "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    m = float(db.sum() + te_codes.sum())
    assert res["mAP"] == m and res["mAP_expected"] == m + 0.5 and res["mAP_expected_bin"] == 2 * m + 0.5
    assert res["precisions_expected"] == [m + 0.25] * 2 and res["recalls_expected"] == [m - 0.25] * 2
    assert [s for s in seen if s[0] == (5, 12)] == [((5, 12), tie, True)] * 2
    assert len(seen) == (8 if concept else 2) and all(s[2] and not s[1] for s in seen if s[0] != (5, 12))
    assert ("mAP_tie_low" in res) == tie and ("mAP_concept" in res) == concept == ("mAP_concept_expected" in res)
    if concept:
        want = [float(db[:, 4 * c:4 * c + 4].sum() + te_codes[:, 4 * c:4 * c + 4].sum()) + 0.5 for c in range(3)]
        assert res["mAP_concept_expected"] == want and len(res["mAP_concept_expected_bin"]) == 3
    assert json.load(open(tmp_path / "history.json")) == res
    assert utils.hashing.calculate_mAP is metric and base.calculate_mAP is metric
    ev.config["tie_expected"] = False                           # the key off: exactly the keys of before
    off = ev.main()
    assert not [k for k in off if "expected" in k] and all(not s[2] for s in seen[-2:])


def test_rescoring_evaluators_drop_the_key_and_keep_what_the_hamming_call_left(tmp_path, monkeypatch):
    """under asymmetric_eval the repeated call must not carry tie_expected (its rank refuses it), and what the Hamming call left in
    utils.hashing.last_tie_expected is what the tie-expectation evaluator reads afterwards"""
    import experiments.test_hashing as base
    import utils.hashing
    from concepthash_amd.config import _wrap
    from experiments.asymmetric_eval import AsymmetricEvaluation
    seen = []

    def metric(db_codes, db_labels, test_codes, test_labels, R, tie_expected=False, PRs=None, rank="hamming", **k):
        seen.append((rank, bool(tie_expected)))
        assert not (tie_expected and rank != "hamming")
        m = float(db_codes.sum()) + (0.25 if rank != "hamming" else 0.0)
        utils.hashing.last_tie_expected = {"mAP_expected": m + 0.5, "precisions_expected": [m] * len(PRs),
                                           "recalls_expected": [m] * len(PRs)} if tie_expected else None
        return m, [m] * len(PRs), [-m] * len(PRs)
    monkeypatch.setattr(utils.hashing, "calculate_mAP", metric)
    monkeypatch.setattr(base, "calculate_mAP", metric)
    db = torch.arange(20, dtype=torch.float32).reshape(5, 4)

    def evaluator_main(self):
        res = {}
        res["mAP"], res["recalls"], res["precisions"] = base.calculate_mAP(db, None, db[:2], None, -1, PRs=[1], threshold=0)
        self.results = res
        return res
    monkeypatch.setattr(base.RetrievalEvaluation, "main", evaluator_main)
    ev = AsymmetricEvaluation.__new__(AsymmetricEvaluation)
    ev.config = _wrap({"asymmetric_eval": True, "weight_bits": 4, "hash_lookup_radii": None, "concept_eval": False, "compute_mAP": True,
                       "exp": "validation", "tie_bracket": False, "tie_expected": True, "sub_code_eval": False, "model": {"ncontext": 3}})
    ev.rank, ev.eval_logdir = 0, str(tmp_path)
    res = ev.main()
    assert seen == [("hamming", True), ("asymmetric", False)]
    assert res["mAP_expected"] == float(db.sum()) + 0.5 and res["mAP_asymmetric"] == float(db.sum()) + 0.25
