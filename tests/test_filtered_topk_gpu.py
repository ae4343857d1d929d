"""GPU: filtered search -- ch_hamming_topk_filtered, ch_hamming_topk_weighted_filtered and ch_ternary_topk_filtered against the numpy
reference (tests/filtered_topk_ref.py) at the smallest shapes that reach every path of the filtered scan, `GalleryIndex.search` under a
filter, and `main_v2.py --config-name search.yaml` with the filter keys on a synthetic run directory.  All arithmetic is integer: every
comparison is exact.  Codes are clustered (a few centres, few flipped bits), so equal distances are the rule and the (distance, index)
order is what is tested."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import filtered_topk_ref as ref
import ternary_ref as tref
import weighted_topk_ref as wref
from conftest import ROOT

pytestmark = pytest.mark.gpu

G_BIG = 140_001           # Qn <= 256: segments of 274 rows for k <= 16 and of 547 at k = 128 -- blocks and segments straddle bitmap words
QN_BIG = 40


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    a = np.array(a)                      # a writable copy: the shared problems are read-only
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dev)


def _same(got, want):
    return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


def _equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _real(rng, rows, nbit, centres):
    """clustered real codes: a centre's signs with 3 flipped bits, magnitudes in (0.05, 1.05)"""
    sign = centres[rng.integers(0, centres.shape[0], rows)].copy()
    flip = rng.integers(0, nbit, (rows, 3))
    for t in range(3):
        sign[np.arange(rows), flip[:, t]] *= -1
    return (sign * (0.05 + rng.random((rows, nbit)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _problem(nbit, Qn, G):
    """(query codes, gallery codes, packed q, packed g, plain distances): computed once and shared; nobody writes to it"""
    rng = np.random.default_rng(7 * nbit + 3 * Qn + G)
    centres = rng.choice(np.array([-1.0, 1.0]), (5, nbit))
    qc, gc = _real(rng, Qn, nbit, centres), _real(rng, G, nbit, centres)
    if G >= Qn:
        gc[:Qn] = qc                                  # every query is also a database row: its own row is at distance 0
    q, g = wref.pack_sign(qc), wref.pack_sign(gc)
    out = (qc, gc, q, g, ref.hamming(q, g))
    for a in out:
        a.setflags(write=False)
    return out


def _allow_lists(rng, G, k, seg):
    """name -> bool [G]: the allow-lists of the issue"""
    runs = np.zeros((G + 63) // 64, bool)
    runs[rng.permutation(runs.size)[:max(1, runs.size // 3)]] = True
    few = np.zeros((G + 63) // 64, bool)                 # fewer admitted rows than k wherever k > 64: one run
    few[rng.integers(0, few.size)] = True
    lists = {"all": np.ones(G, bool), "none": np.zeros(G, bool), "random 0.5": rng.random(G) < 0.5, "random 0.01": rng.random(G) < 0.01,
             "runs of 64": np.repeat(runs, 64)[:G], "one run": np.repeat(few, 64)[:G]}
    for name, r in (("first", 0), ("last", G - 1), ("segment start", seg if seg < G else 0), ("tail", max(0, G - 2))):
        one = np.zeros(G, bool)
        one[r] = True
        lists["only row " + name] = one
    return lists


def _seg_rows(Qn, G, k):
    """the plain scan's segment length for Qn <= 256 (csrc/hamming_shared.h, topk_seg_rows_for): where the tests put a segment start"""
    per_cu = 8 if k <= 16 else 7 if k <= 32 else 3 if k <= 64 else 1
    nseg = max(1, min(256 * per_cu, max(512, G // 4096)))
    return max(256, -(-G // nseg))


# ---- every row admitted: the unfiltered entries, bit for bit -------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 10, 16, 32, 64, 128])
@pytest.mark.parametrize("nbit", [64, 128, 200])
def test_with_every_row_admitted_the_lists_are_the_unfiltered_ones(dev, nbit, k):
    from concepthash_amd import retrieval as rt
    Qn, G = 257, 771
    qc, gc, q, g, _ = _problem(nbit, Qn, G)
    tq, tg, tqc = _t(q, dev), _t(g, dev), _t(qc, dev)
    rng = np.random.default_rng(k)
    shared = _t(rng.integers(0, 1 << 63, ((nbit + 63) // 64,), dtype=np.uint64), dev)
    per = rt.confidence_mask(tqc, 0.3)
    ones = torch.ones(G, dtype=torch.bool, device=dev)
    nobody = torch.full((Qn,), -1, dtype=torch.int64, device=dev)
    garbage = _t(ref.pack_allow(np.ones(G, bool), garbage=True), dev)
    for allow, want in ((ones, None), (garbage, None), (None, nobody), (ones, nobody), (None, None)):
        kw = dict(allow=allow, want=want)
        assert _equal(rt.hamming_topk_filtered(tq, tg, k, **kw), rt.hamming_topk(tq, tg, k))
        for mask in (shared, per):
            assert _equal(rt.hamming_topk_filtered(tq, tg, k, mask=mask, **kw), rt.hamming_topk_masked(tq, tg, mask, k))
        for bits in (4, 8):
            planes = rt.weight_planes(tqc, bits)[0]
            assert _equal(rt.hamming_topk_filtered(tq, tg, k, planes=planes, **kw), rt.hamming_topk_weighted(tq, planes, tg, k))
        q3, g3 = rt.pack_ternary(tqc, 0.3), rt.pack_ternary(_t(gc, dev), 0.2)
        assert _equal(rt.ternary_topk_filtered(q3, g3, nbit, k, **kw), rt.ternary_topk(q3, g3, nbit, k))


# ---- allow-lists ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbit,k,Qn,G", [(64, 1, 1, 1), (64, 10, 70, 207), (128, 16, 257, 771), (200, 32, 70, 771), (64, 64, 1, 771),
                                         (200, 128, 257, 207), (128, 128, 70, 771), (64, 10, 257, 771)])
def test_allow_lists_against_the_reference(dev, nbit, k, Qn, G):
    from concepthash_amd import retrieval as rt
    _, _, q, g, D = _problem(nbit, Qn, G)
    tq, tg = _t(q, dev), _t(g, dev)
    rng = np.random.default_rng(nbit + k + G)
    for name, allow in _allow_lists(rng, G, k, 256).items():
        want = ref.topk(D, ref.admitted(Qn, G, allow=allow), k)
        if name == "none":
            assert (want[0] == -1).all() and (want[1] == -1).all()
        if name == "one run" and k > 64:
            assert (want[0][:, -1] == -1).all() and (want[0][:, 0] >= 0).all()              # a -1 tail behind real hits
        assert _same(rt.hamming_topk_filtered(tq, tg, k, allow=_t(allow, dev)), want), name
        for garbage in (False, True):                                                       # packed, with ones past G in the last word
            packed = _t(ref.pack_allow(allow, garbage=garbage), dev)
            assert _same(rt.hamming_topk_filtered(tq, tg, k, allow=packed), want), (name, garbage)


@functools.lru_cache(maxsize=None)
def _big():
    return _problem(64, QN_BIG, G_BIG)


@pytest.mark.parametrize("k", [10, 128])
def test_segments_and_blocks_that_straddle_bitmap_words(dev, k):
    """140,001 rows: segments of 274 (k = 10) and 547 (k = 128) rows, no multiple of 4 or of 64"""
    from concepthash_amd import retrieval as rt
    _, _, q, g, D = _big()
    Qn, G = QN_BIG, G_BIG
    seg = _seg_rows(Qn, G, k)
    assert seg == (274 if k == 10 else 547)
    tq, tg = _t(q, dev), _t(g, dev)
    rng = np.random.default_rng(k)
    runs = rng.random((G + 63) // 64) < 0.01
    one = np.zeros(G, bool)
    one[3 * seg] = True                                                                     # the first row of the fourth segment
    tail = np.zeros(G, bool)
    tail[[seg - 1, 2 * seg - 2, G - 1]] = True                                              # rows of the one-row tail loops
    base = 10 ** 6
    own = base + np.arange(Qn, dtype=np.int64)
    group = (rng.integers(0, 5, G)).astype(np.int32)
    for name, allow in (("random 0.5", rng.random(G) < 0.5), ("runs of 64, 0.01", np.repeat(runs, 64)[:G]), ("segment start", one),
                        ("tails", tail)):
        assert _same(rt.hamming_topk_filtered(tq, tg, k, allow=_t(allow, dev), g_index_base=base),
                     ref.topk(D, ref.admitted(Qn, G, allow=allow), k, base)), name
        adm = ref.admitted(Qn, G, allow=allow, want=own, exclude=True, base=base)
        assert _same(rt.hamming_topk_filtered(tq, tg, k, allow=_t(allow, dev), want=_t(own, dev), exclude=True, g_index_base=base),
                     ref.topk(D, adm, k, base)), name
        want = np.arange(Qn, dtype=np.int64) % 6 - 1                                        # -1 .. 4
        adm = ref.admitted(Qn, G, allow=allow, group=group, want=want)
        assert _same(rt.hamming_topk_filtered(tq, tg, k, allow=_t(allow, dev), group=_t(group, dev), want=_t(want, dev)),
                     ref.topk(D, adm, k)), name


# ---- the group part ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbit,k,Qn,G", [(64, 10, 70, 771), (128, 32, 257, 771), (200, 128, 70, 207), (64, 16, 1, 207)])
def test_group_filter_against_the_reference(dev, nbit, k, Qn, G):
    from concepthash_amd import retrieval as rt
    _, _, q, g, D = _problem(nbit, Qn, G)
    tq, tg = _t(q, dev), _t(g, dev)
    rng = np.random.default_rng(nbit + k)
    group = rng.integers(0, 5, G).astype(np.int32)
    want = rng.integers(0, 5, Qn).astype(np.int64)
    some = want.copy()
    some[::3] = -1                                                                          # no group filter for these queries
    nobody = np.full(Qn, 7, np.int64)                                                       # a group no row has
    far = np.full(Qn, (1 << 40) + 3, np.int64)                                              # ... and one that no int32 holds
    plain = rt.hamming_topk(tq, tg, k)
    for exclude in (False, True):
        for w in (want, some):
            adm = ref.admitted(Qn, G, group=group, want=w, exclude=exclude)
            assert _same(rt.hamming_topk_filtered(tq, tg, k, group=_t(group, dev), want=_t(w, dev), exclude=exclude), ref.topk(D, adm, k))
        for w in (nobody, far):
            got = rt.hamming_topk_filtered(tq, tg, k, group=_t(group, dev), want=_t(w, dev), exclude=exclude)
            if exclude:
                assert _equal(got, plain)
            else:
                assert bool((got[0] == -1).all()) and bool((got[1] == -1).all())
    # no plane: a row is its own group, numbered from the base.  The queries are the first Qn database rows
    for base in (0, 10 ** 6):
        own = base + np.arange(Qn, dtype=np.int64)
        own[1::4] = -1
        if G < Qn:
            own[G:] = -1
        got = rt.hamming_topk_filtered(tq, tg, k, want=_t(own, dev), exclude=True, g_index_base=base)
        assert _same(got, ref.topk(D, ref.admitted(Qn, G, want=own, exclude=True, base=base), k, base))
        # the query's own row disappears and everything else is as unfiltered: the unfiltered k + 1 list without that row
        if k < 128:
            idx1, dst1 = (t.cpu().numpy() for t in rt.hamming_topk(tq, tg, k + 1, g_index_base=base))
            for i in range(Qn):
                keep = idx1[i] != own[i]
                assert np.array_equal(got[0][i].cpu().numpy(), idx1[i][keep][:k]) and np.array_equal(got[1][i].cpu().numpy(), dst1[i][keep][:k])
                assert own[i] < 0 or own[i] not in got[0][i].cpu().numpy()
        only = rt.hamming_topk_filtered(tq, tg, k, want=_t(own, dev), g_index_base=base)
        assert _same(only, ref.topk(D, ref.admitted(Qn, G, want=own, base=base), k, base))
        outside = _t(np.full(Qn, base + G, np.int64), dev)                                    # the row behind the gallery: nobody's
        assert _equal(rt.hamming_topk_filtered(tq, tg, k, want=outside, exclude=True, g_index_base=base),
                      rt.hamming_topk(tq, tg, k, g_index_base=base))


def test_both_parts_at_once(dev):
    from concepthash_amd import retrieval as rt
    nbit, k, Qn, G = 128, 16, 257, 771
    _, _, q, g, D = _problem(nbit, Qn, G)
    tq, tg = _t(q, dev), _t(g, dev)
    rng = np.random.default_rng(11)
    group = rng.integers(0, 5, G).astype(np.int32)
    want = rng.integers(-1, 5, Qn).astype(np.int64)
    for name, allow in _allow_lists(rng, G, k, 256).items():
        for exclude in (False, True):
            adm = ref.admitted(Qn, G, allow=allow, group=group, want=want, exclude=exclude)
            got = rt.hamming_topk_filtered(tq, tg, k, allow=_t(allow, dev), group=_t(group, dev), want=_t(want, dev), exclude=exclude)
            assert _same(got, ref.topk(D, adm, k)), (name, exclude)


# ---- masks, planes, ternary codes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbit,k,Qn,G", [(64, 10, 70, 771), (200, 32, 257, 207), (128, 128, 70, 771)])
def test_masked_weighted_and_ternary_under_the_same_filter(dev, nbit, k, Qn, G):
    from concepthash_amd import retrieval as rt
    qc, gc, q, g, _ = _problem(nbit, Qn, G)
    tq, tg = _t(q, dev), _t(g, dev)
    rng = np.random.default_rng(nbit + G)
    W = (nbit + 63) // 64
    allow = rng.random(G) < 0.5
    group = rng.integers(0, 5, G).astype(np.int32)
    want = rng.integers(-1, 5, Qn).astype(np.int64)
    filters = [dict(allow=allow), dict(group=group, want=want, exclude=True), dict(allow=allow, group=group, want=want, exclude=False)]
    shared = rng.integers(0, 1 << 63, (W,), dtype=np.uint64)
    per = rng.integers(0, 1 << 63, (Qn, W), dtype=np.uint64)
    if nbit % 64:                                                                           # the codes' last word is zero past nbit
        per[:, -1] &= np.uint64((1 << (nbit % 64)) - 1)
    dists = [(dict(mask=_t(m, dev)), ref.hamming(q, g, m)) for m in (shared, per)]
    for bits in (4, 8):
        w = wref.weights(qc, bits)
        dists.append((dict(planes=_t(wref.planes_of(w, bits), dev)), ref.weighted(q, g, w)))
    for f in filters:
        adm = ref.admitted(Qn, G, **f)
        tf = {n: (_t(v, dev) if isinstance(v, np.ndarray) else v) for n, v in f.items()}
        for kw, D in dists:
            assert _same(rt.hamming_topk_filtered(tq, tg, k, **kw, **tf), ref.topk(D, adm, k)), (sorted(kw), sorted(f))
        pq, pg = tref.planes(tref.ternarise(qc, 0.3)), tref.planes(tref.ternarise(gc, 0.2))
        K = ref.ternary(pq, pg, nbit)
        assert _same(rt.ternary_topk_filtered(_t(pq, dev), _t(pg, dev), nbit, k, **tf), ref.topk(K, adm, k)), sorted(f)


# ---- shards --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 64])
def test_two_unequal_shards_merge_into_the_whole_call(dev, k):
    from concepthash_amd import retrieval as rt
    nbit, Qn, G, cut, base = 128, 70, 771, 301, 5000
    qc, gc, q, g, D = _problem(nbit, Qn, G)
    tq, tg = _t(q, dev), _t(g, dev)
    rng = np.random.default_rng(k)
    allow = rng.random(G) < 0.3
    group = rng.integers(0, 5, G).astype(np.int32)
    want = rng.integers(-1, 5, Qn).astype(np.int64)
    own = base + np.arange(Qn, dtype=np.int64)
    q3, g3 = rt.pack_ternary(_t(qc, dev), 0.3), rt.pack_ternary(_t(gc, dev), 0.2)
    for f in (dict(allow=allow, group=group, want=want, exclude=False), dict(allow=allow, want=own, exclude=True)):
        def call(fn, codes, lo, hi, *a):
            kw = dict(allow=_t(f["allow"][lo:hi], dev), want=_t(f["want"], dev), exclude=f["exclude"], g_index_base=base + lo)
            if "group" in f:
                kw["group"] = _t(f["group"][lo:hi], dev)
            return fn(a[0], codes[lo:hi], *a[1:], **kw)
        for fn, qq, gg, a in ((rt.hamming_topk_filtered, tq, tg, (k,)), (rt.ternary_topk_filtered, q3, g3, (nbit, k))):
            whole = call(fn, gg, 0, G, qq, *a)
            parts = [call(fn, gg, 0, cut, qq, *a), call(fn, gg, cut, G, qq, *a)]
            merged = rt.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
            assert _equal(merged, whole)
        adm = ref.admitted(Qn, G, base=base, **f)
        assert _same(call(rt.hamming_topk_filtered, tg, 0, G, tq, k), ref.topk(D, adm, k, base))


def test_a_shard_without_an_admitted_row_merges_as_empty_lists(dev):
    """topk_merge with a list that is empty throughout: one shard's lists are all -1, the other's hold 10 hits and 6 x -1"""
    from concepthash_amd import retrieval as rt
    nbit, Qn, G, cut, k = 64, 3, 771, 301, 16
    _, _, q, g, D = _problem(nbit, Qn, G)
    tq, tg = _t(q, dev), _t(g, dev)
    allow = np.zeros(G, bool)
    allow[np.random.default_rng(16).permutation(np.arange(cut, G))[:10]] = True
    parts = [rt.hamming_topk_filtered(tq, tg[lo:hi], k, allow=_t(allow[lo:hi], dev), g_index_base=lo) for lo, hi in ((0, cut), (cut, G))]
    assert (parts[0][0] == -1).all() and (parts[0][1] == -1).all()
    assert ((parts[1][0] >= 0).sum(1) == 10).all() and (parts[1][0][:, 10:] == -1).all()
    want = ref.topk(D, ref.admitted(Qn, G, allow=allow), k)
    for order in (parts, parts[::-1]):
        assert _same(rt.topk_merge(torch.stack([p[0] for p in order]), torch.stack([p[1] for p in order])), want)


# ---- GalleryIndex.search -------------------------------------------------------------------------------------------------------------

def _index(dev, labels, nbit=64, Qn=70, G=771):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    qc, gc, q, g, D = _problem(nbit, Qn, G)
    rng = np.random.default_rng(5)
    if labels == "single":
        lab = torch.from_numpy(rng.integers(0, 6, G))
    else:
        lab = torch.from_numpy((rng.random((G, 6)) < 0.3).astype(np.uint8))
    tg = _t(gc, dev)
    groups = torch.from_numpy(rng.integers(0, 4, G).astype(np.int32))
    index = GalleryIndex(rt.pack_sign(tg), nbit, 4, labels=lab.to(dev), mask=rt.confidence_mask(tg, 0.2), margin=0.2,
                         groups=groups.to(dev))
    return index, qc, gc, q, g, D, lab.numpy(), groups.numpy()


@pytest.mark.parametrize("labels", ["single", "rows"])
def test_search_by_classes_against_the_reference(dev, labels):
    index, qc, gc, q, g, D, lab, _ = _index(dev, labels)
    Qn, G, k = 70, 771, 10
    has = (lambda c: lab == c) if labels == "single" else (lambda c: lab[:, c] != 0)
    rows = np.random.default_rng(1).random(G) < 0.7
    cases = [(dict(labels_in=[1, 4]), has(1) | has(4)), (dict(labels_out=[0, 2, 3]), ~(has(0) | has(2) | has(3))),
             (dict(labels_in=[1, 4, 5], labels_out=[4]), (has(1) | has(4) | has(5)) & ~has(4)),
             (dict(rows=torch.from_numpy(rows), labels_in=[2]), rows & has(2)),
             (dict(rows=_t(ref.pack_allow(rows, garbage=True), dev), labels_out=[2]), rows & ~has(2)),
             (dict(labels_in=[]), np.zeros(G, bool))]
    for kw, allow in cases:
        out = index.search(torch.from_numpy(np.array(qc)), k, **kw)
        assert _same((out["idx"], out["dist"]), ref.topk(D, ref.admitted(Qn, G, allow=allow), k)), sorted(kw)
        assert out["rows_admitted"] == int(allow.sum())
        hit = out["idx"].cpu().numpy()
        assert allow[hit[hit >= 0]].all()
        assert np.array_equal(out["concept_dist"].cpu().numpy().sum(2)[hit >= 0], out["dist"].cpu().numpy()[hit >= 0])


def test_search_without_the_query_itself_and_by_groups(dev):
    index, qc, gc, q, g, D, lab, groups = _index(dev, "single")
    Qn, G, k = 70, 771, 10
    tqc = torch.from_numpy(np.array(qc))
    own = torch.arange(Qn, dtype=torch.int64)                                               # query i is database row i
    out = index.search(tqc, k, query_group=own, group_mode="exclude", group_by="row")
    assert _same((out["idx"], out["dist"]), ref.topk(D, ref.admitted(Qn, G, want=own.numpy(), exclude=True), k))
    assert out["rows_admitted"] == G and not bool((out["idx"] == own[:, None].to(dev)).any())
    plain = index.search(tqc, k + 1)
    assert "rows_admitted" not in plain and bool((plain["idx"][:, 0] == own.to(dev)).all())  # unfiltered, every query finds itself first
    assert torch.equal(out["idx"], plain["idx"][:, 1:]) and torch.equal(out["dist"], plain["dist"][:, 1:])
    want = torch.from_numpy(np.random.default_rng(2).integers(-1, 4, Qn))
    for mode in ("only", "exclude"):
        out = index.search(tqc, k, query_group=want, group_mode=mode)
        assert _same((out["idx"], out["dist"]), ref.topk(D, ref.admitted(Qn, G, group=groups, want=want.numpy(), exclude=mode == "exclude"), k))
        ql = torch.from_numpy(lab[:Qn].astype(np.int64))                                    # same class only / another class only
        out = index.search(tqc, k, query_group=ql, group_mode=mode, group_by="labels")
        assert _same((out["idx"], out["dist"]), ref.topk(D, ref.admitted(Qn, G, group=lab, want=ql.numpy(), exclude=mode == "exclude"), k))
        same = out["labels"].cpu().numpy() == ql.numpy()[:, None]
        assert same[out["idx"].cpu().numpy() >= 0].all() if mode == "only" else not same.any()


@pytest.mark.parametrize("rank", ["hamming", "asymmetric", "ternary"])
def test_search_filter_composes_with_concepts_margin_and_radius(dev, rank):
    from concepthash_amd import retrieval as rt
    index, qc, gc, q, g, _, lab, groups = _index(dev, "single")
    Qn, G, k, nbit = 70, 771, 16, 64
    tqc = torch.from_numpy(np.array(qc))
    allow = (lab == 1) | (lab == 3) | (lab == 5)
    want = np.random.default_rng(3).integers(-1, 4, Qn).astype(np.int64)
    adm = ref.admitted(Qn, G, allow=allow, group=groups, want=want, exclude=True)
    kw = dict(labels_in=[1, 3, 5], query_group=torch.from_numpy(want), group_mode="exclude")
    concepts, margin = [0, 2], 0.3
    cmask = rt.concept_mask(nbit, 4, concepts).numpy().view(np.uint64)
    for cs, m, radius in ((None, 0.0, None), (concepts, 0.0, None), (None, margin, None), (concepts, margin, 3)):
        if rank == "asymmetric" and radius is not None:
            radius = None
        out = index.search(tqc, k, cs, m, rank=rank, weight_bits=4, radius=radius, **kw)
        mask = None if cs is None else cmask
        if rank == "ternary":
            pq = tref.planes(tref.ternarise(qc, m))
            pg = tref.planes(tref.ternarise(gc, 0.2))
            play = nbit if cs is None else 32
            D = ref.ternary(pq if cs is None else pq & cmask[None, None, :], pg, play)
            cut = None if radius is None else 2 * radius
        else:
            if m > 0:
                conf = tref.confidence_mask(qc, m)
                mask = conf if mask is None else conf & mask[None, :]
            D = ref.hamming(q, g, mask) if rank == "hamming" else ref.weighted(q, g, wref.weights(qc, 4, mask))
            cut = radius
        idx, dst = ref.topk(D, adm, k)
        if cut is not None:                                                                 # the radius cuts after the filter
            far = dst > cut
            idx[far], dst[far] = -1, -1
        assert _same((out["idx"], out["dist"]), (idx, dst)), (rank, cs, m, radius)
        assert out["rows_admitted"] == int(allow.sum())


# ---- the command ---------------------------------------------------------------------------------------------------------------------

COMMON = ["dataset=synthetic_cub200", "dataset.limit=96", "batch_size=32"]


def _main_v2(args, cwd):
    subprocess.run([sys.executable, os.path.join(ROOT, "main_v2.py")] + args, check=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=cwd,
                   timeout=600)


def test_search_command_excludes_the_query_itself_and_keeps_to_classes(tmp_path, dev):
    """a synthetic run directory, built as tests/test_search_gpu.py builds its own"""
    from concepthash_amd.search import GalleryIndex
    tmp = tmp_path
    logdir = str(tmp / "run")
    common = COMMON + ["data_dir=" + str(tmp)]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_logdir.py"), logdir,
                    "model.backbone.name=synthetic/clip-vit-small-patch16", "model.nbit=64"] + common, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp))
    s1, s2, s3 = str(tmp / "s1"), str(tmp / "s2"), str(tmp / "s3")
    search = ["--config-name", "search.yaml", "logdir=" + logdir, "query=db"] + common
    _main_v2(search + ["search_logdir=" + s1, "k=6"], str(tmp))
    _main_v2(search + ["search_logdir=" + s2, "k=5", "exclude_self=true"], str(tmp))
    plain = json.load(open(os.path.join(s1, "results.json")))
    res = json.load(open(os.path.join(s2, "results.json")))
    assert plain["filter"] is None and res["k"] == 5
    assert res["filter"] == {"only_classes": None, "exclude_classes": None, "exclude_self": True, "same_class": None,
                             "rows_admitted": res["index_rows"]}
    assert len(res["queries"]) == len(plain["queries"]) == res["index_rows"] > 6
    for i, (e, p) in enumerate(zip(res["queries"], plain["queries"])):
        hits = [(h["index"], h["distance"]) for h in e["hits"]]
        assert i not in [h[0] for h in hits] and len(hits) == 5
        assert hits == [(h["index"], h["distance"]) for h in p["hits"] if h["index"] != i][:5], i   # the k = 6 list without that row
    index = GalleryIndex.load(os.path.join(logdir, "index_best.pth"))
    classes = sorted(set(index.labels.tolist()))[:3]
    _main_v2(search + ["search_logdir=" + s3, "k=5", "only_classes=[" + ",".join(str(c) for c in classes) + "]"], str(tmp))
    res = json.load(open(os.path.join(s3, "results.json")))
    admitted = int(sum(int(l) in classes for l in index.labels.tolist()))
    assert res["filter"] == {"only_classes": classes, "exclude_classes": None, "exclude_self": False, "same_class": None,
                             "rows_admitted": admitted} and 0 < admitted < res["index_rows"]
    for e in res["queries"]:
        assert len(e["hits"]) == min(5, admitted) and all(h["label"] in classes for h in e["hits"])
