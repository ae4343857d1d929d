"""GPU: ranked lists of any depth and hash lookup (csrc/hamming_rank.hip through retrieval.hamming_ranked / hamming_radius,
GalleryIndex.search and evaluate(radii=...)) -- bit for bit against the stable argsort of the full distance matrix (tests/ranked_ref.py),
against the C oracle's counting sort and against the top-k scan: three algorithms, one ranking."""
import functools

import numpy as np
import pytest
import torch

import ranked_ref as rr

pytestmark = pytest.mark.gpu

NCENTRES = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.array(a, copy=True)).to(dev)       # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def _case(W, Qn, G):
    """Clustered codes (3 centres, flip 0.1): distance buckets hundreds of rows deep, so every k cuts a tie that spans segments; the last
    rows of the gallery are exact duplicates of query 0.  -> (q, g, order, sorted distances): computed once per shape, never changed."""
    nbit = 64 * W
    centres = np.random.default_rng(100 + W).integers(0, 2, (NCENTRES, nbit)).astype(np.uint8)
    g = rr.clustered(np.random.default_rng(G).integers(0, NCENTRES, G), centres, nbit, 7 * G + W)
    q = rr.clustered(np.arange(Qn) % NCENTRES, centres, nbit, 13 * Qn + W)
    g[-min(3, G):] = q[0]
    order, ds, _ = rr.ranking(q, g)
    for a in (q, g, order, ds):
        a.setflags(write=False)
    return q, g, order, ds


def _slice(order, ds, k, base=0):
    Qn, G = order.shape
    idx = np.full((Qn, k), -1, dtype=np.int64)
    dist = np.full((Qn, k), -1, dtype=np.int32)
    n = min(k, G)
    idx[:, :n], dist[:, :n] = order[:, :n] + base, ds[:, :n]
    return idx, dist


def _same(got, want):
    return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_ranked_lists_equal_the_stable_argsort_on_the_shape_grid(dev, W):
    """Qn 1 / 70 / 257 (one lane, a ragged tile, two or three tiles) x G around one, two and three trips of four and of eight rows and
    over several segments x seg_rows 256 / 257 (a ragged last segment: ranks carry across segments) x k from 1 to past the gallery."""
    from concepthash_amd import retrieval as rt
    from oracle import hamming_oracle as ho
    for Qn in (1, 70, 257):
        for G in (1, 7, 8, 9, 15, 16, 17, 24, 25, 1000, 4100):
            q, g, order, ds = _case(W, Qn, G)
            tq, tg = _t(q, dev), _t(g, dev)
            for k in sorted({1, 129, 1000, G, G + 5}):
                want = _slice(order, ds, k)
                ridx, rdst = ho.topk(q, g, k)
                assert np.array_equal(want[0], ridx.astype(np.int64)) and np.array_equal(want[1], rdst)
                for seg in (256, 257):
                    assert _same(rt.hamming_ranked(tq, tg, k, seg_rows=seg), want), (W, Qn, G, k, seg)


@pytest.mark.parametrize("W", [1, 3])
def test_every_exit_of_the_scalar_block_walk_in_both_of_its_users(dev, W):
    """The scalar double-buffered walk over a segment -- load a block, scan the previous one, the odd-block case, the row tail -- is
    written in the two-scan mAP passes (blocks of 4 rows; taken under the scalar-load tap) and in the rank pass (blocks of 8 rows at
    W <= 2, of 4 above).  Segments of 3 / 4 / 8 / 9 / 16 / 25 rows are shorter than a block, exactly one block, two blocks, and odd
    whole blocks plus a tail for one block size or the other; the gallery's last segment is ragged.  evaluate(records=False) in the
    VMEM form and the scalar form against the oracle, hamming_ranked for a short and a past-the-gallery k against the stable argsort."""
    from concepthash_amd import _lib, retrieval as rt
    from oracle import hamming_oracle as ho
    lib = _lib.load()
    Qn, G = 70, 130 if W == 3 else 100
    q, ql = ho.synthetic_codes(Qn, 64 * W, seed=71, nclass=5, flip=0.15)
    g, gl = ho.synthetic_codes(G, 64 * W, seed=72, nclass=5, flip=0.15)
    ref = ho.mean_ap(q, g, ql, gl, R=-1, ks=(1, 5, 10), remove_first=False)
    order, ds, _ = rr.ranking(q, g)
    tq, tg, tql, tgl = _t(q, dev), _t(g, dev), _t(ql, dev), _t(gl, dev)
    for seg in (3, 4, 8, 9, 16, 25):
        for scalar in (0, 1):
            lib.ch_debug_set_hamming_scalar_loads(scalar)
            try:
                got = rt.evaluate(tq, tg, tql, tgl, R=-1, ks=(1, 5, 10), seg_rows=seg, records=False)
            finally:
                lib.ch_debug_set_hamming_scalar_loads(0)
            assert np.array_equal(got["S"].cpu().numpy().view(np.uint64), ref["S"]), (seg, scalar)
            for key in ("nrel", "hits", "total"):
                assert np.array_equal(got[key].cpu().numpy().astype(np.uint32), ref[key]), (seg, scalar, key)
        for k in (7, G + 3):
            assert _same(rt.hamming_ranked(tq, tg, k, seg_rows=seg), _slice(order, ds, k)), (seg, k)


def test_ranked_lists_with_the_default_segments(dev):
    from concepthash_amd import retrieval as rt
    q, g, order, ds = _case(1, 700, 9001)
    assert 9001 // rt.map_seg_rows(700, 9001, 1) >= 2                   # several segments
    tq, tg = _t(q, dev), _t(g, dev)
    for k in (1000, 9001):
        assert _same(rt.hamming_ranked(tq, tg, k), _slice(order, ds, k)), k


def test_ties_duplicates_index_base_determinism_and_fill(dev):
    from concepthash_amd import retrieval as rt
    q, g, order, ds = _case(1, 70, 4100)
    tq, tg = _t(q, dev), _t(g, dev)
    base = 5_000_000_000                                                # past 2^32: the index is 64-bit
    # the duplicates of query 0 close the gallery and open its list, in gallery order
    assert np.array_equal(order[0, :3], [4097, 4098, 4099]) and (ds[0, :3] == 0).all()
    # k = 700 cuts, for every query, a bucket more than a hundred rows deep whose rows lie in most of the 17 segments
    tied = ds == ds[:, 699][:, None]
    assert (tied.sum(1) > 100).all() and all(len(set(order[i][tied[i]] // 256)) > 8 for i in range(70))
    for k in (129, 700):
        a = rt.hamming_ranked(tq, tg, k, g_index_base=base, seg_rows=256)
        b = rt.hamming_ranked(tq, tg, k, g_index_base=base, seg_rows=256)
        assert _same(a, _slice(order, ds, k, base)), k
        assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    idx, dist = rt.hamming_ranked(tq, tg, 4300, seg_rows=257)
    assert (idx[:, 4100:] == -1).all() and (dist[:, 4100:] == -1).all() and (idx[:, :4100] >= 0).all()
    idx, dist = rt.hamming_ranked(tq, tg[:0], 5)                        # an empty gallery: all fill
    assert idx.shape == (70, 5) and (idx == -1).all() and (dist == -1).all()
    assert rt.hamming_ranked(tq[:0], tg, 5)[0].shape == (0, 5)
    # the entry itself: limits that reach past the buffers are refused before the launch
    _, base, counts = rt.bucket_counts(tq, tg, 256)
    assert counts.shape == (70, 65) and (counts.sum(1) == 4100).all()
    out_i, out_d = torch.empty(70 * 4, dtype=torch.int64, device=dev), torch.empty(70 * 4, dtype=torch.int32, device=dev)
    start = torch.arange(70, device=dev) * 4
    with pytest.raises(ValueError, match="outside"):
        rt.rank_scatter(tq, tg, 256, base, start, torch.full((70,), 5, device=dev), out_i, out_d)
    rt.rank_scatter(tq, tg, 256, base, start, torch.full((70,), 4, device=dev), out_i, out_d)
    assert np.array_equal(out_i.cpu().numpy().reshape(70, 4), order[:, :4]) and np.array_equal(out_d.cpu().numpy().reshape(70, 4), ds[:, :4])


@pytest.mark.parametrize("W", [1, 2, 4])
def test_ranked_lists_agree_with_the_topk_scan(dev, W):
    from concepthash_amd import retrieval as rt
    q, g, _, _ = _case(W, 257, 4100)
    tq, tg = _t(q, dev), _t(g, dev)
    for k in (10, 128):
        a, b = rt.hamming_ranked(tq, tg, k, g_index_base=77), rt.hamming_topk(tq, tg, k, g_index_base=77)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k


@pytest.mark.parametrize("W", [1, 3])
def test_radius_search_equals_the_restatement(dev, W):
    from concepthash_amd import retrieval as rt
    q, g, order, ds = _case(W, 70, 4100)
    q = q.copy()
    q[5] = ~g[0]                                                        # far from its cluster: its small-radius lists are empty
    tq, tg = _t(q, dev), _t(g, dev)
    _, ds5, _ = rr.ranking(q[5:6], g)
    assert ds5[0, 0] > 2
    mid = int(np.median(ds[:, 0::7]))
    for radius in (0, 2, mid, 64 * W):
        for max_hits, base, seg in ((None, 0, 256), (40, 9, 257)):
            want = rr.radius_csr(q, g, radius, g_index_base=base, max_hits=max_hits)
            off, idx, dist = rt.hamming_radius(tq, tg, radius, g_index_base=base, max_hits=max_hits, seg_rows=seg)
            assert np.array_equal(off.cpu().numpy(), want[0]), (radius, max_hits)
            assert np.array_equal(idx.cpu().numpy(), want[1]) and np.array_equal(dist.cpu().numpy(), want[2]), (radius, max_hits)
            if radius <= 2:
                assert off[6] == off[5]                                 # the empty list
    off, idx, dist = rt.hamming_radius(tq, tg, 64 * W)                  # the whole ranking in CSR form
    full, fds, _ = rr.ranking(q, g)
    assert np.array_equal(off.cpu().numpy(), np.arange(71) * 4100) and np.array_equal(idx.cpu().numpy().reshape(70, 4100), full)
    assert np.array_equal(dist.cpu().numpy().reshape(70, 4100), fds)
    # hamming_ranked under a radius: the same rows, -1 behind them
    small = int(ds[:, 299].min()) - 1                                   # some query has fewer than 300 rows this close
    want = rr.ranked(q, g, 300, radius=small)
    assert _same(rt.hamming_ranked(tq, tg, 300, radius=small, seg_rows=256), want) and (want[0] == -1).any() and (want[0][:, 0] >= 0).any()
    off, idx, _ = rt.hamming_radius(tq, tg[:0], 3)
    assert off.tolist() == [0] * 71 and idx.numel() == 0


def test_radius_search_that_retrieves_nothing(dev):
    """No query has a row within the radius (no duplicates in the gallery), or max_hits = 0: zero offsets and empty lists, no launch on
    buffers without an address."""
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(21)
    for W in (1, 2):
        q = rng.integers(0, 2 ** 63, (70, W), dtype=np.int64).view(np.uint64)
        g = rng.integers(0, 2 ** 63, (1000, W), dtype=np.int64).view(np.uint64)
        _, ds, _ = rr.ranking(q, g)
        assert ds[:, 0].min() > 2                                       # uniform codes: nothing within 2 bits
        tq, tg = _t(q, dev), _t(g, dev)
        for radius, max_hits in ((0, None), (2, None), (64 * W, 0)):
            off, idx, dist = rt.hamming_radius(tq, tg, radius, max_hits=max_hits, seg_rows=256)
            assert off.tolist() == [0] * 71 and idx.shape == (0,) and dist.shape == (0,) and idx.dtype == torch.int64 and dist.dtype == torch.int32
        idx, dist = rt.hamming_ranked(tq, tg, 129, radius=2)
        assert (idx == -1).all() and (dist == -1).all()
        # the entry's wrapper with nothing to place
        _, base, _ = rt.bucket_counts(tq, tg, 256)
        zero = torch.zeros(70, dtype=torch.int64, device=dev)
        rt.rank_scatter(tq, tg, 256, base, zero, zero, torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
        # one query with a hit among queries without: the lists before and after it stay empty
        g2 = g.copy()
        g2[500] = q[33]
        off, idx, dist = rt.hamming_radius(tq, _t(g2, dev), 0)
        assert off.tolist() == [0] * 34 + [1] * 37 and idx.tolist() == [500] and dist.tolist() == [0]


def test_shared_mask_and_refused_per_query_mask(dev):
    from concepthash_amd import retrieval as rt
    q, g, _, _ = _case(2, 70, 1000)
    tq, tg = _t(q, dev), _t(g, dev)
    mask = np.array([0x00FFFF0000FFFF00, 0xF0F0F0F0F0F0F0F0], dtype=np.uint64)
    tm = _t(mask, dev)
    for k in (129, 1005):
        assert _same(rt.hamming_ranked(tq, tg, k, mask=tm, seg_rows=256), rr.ranked(q, g, k, mask=mask)), k
    a, b = rt.hamming_ranked(tq, tg, 100, mask=tm), rt.hamming_topk_masked(tq, tg, tm, 100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want = rr.radius_csr(q, g, 9, mask=mask)
    got = rt.hamming_radius(tq, tg, 9, mask=tm)
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got, want))
    with pytest.raises(ValueError, match="per-query mask"):
        rt.hamming_ranked(tq, tg, 129, mask=tm[None, :].expand(70, 2).contiguous())


def test_gallery_index_search_deep_lists_and_radius(dev):
    from concepthash_amd import retrieval as rt
    from concepthash_amd.search import GalleryIndex
    nbit, Q, G, Qn = 128, 4, 1000, 70
    q, g, _, _ = _case(2, Qn, G)
    as_codes = lambda p: np.unpackbits(p.view(np.uint8), axis=1, bitorder="little").astype(np.float32) * 2 - 1
    qc, tg = _t(as_codes(q), dev), _t(g, dev)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 9, G))
    index = GalleryIndex(tg, nbit, Q, labels=labels, paths=[f"img/{i}.jpg" for i in range(G)], data_root="/d").to(dev)
    # k = 300 by concepts 0 and 2: the restatement under their shared mask
    mask = rt.concept_mask(nbit, Q, [0, 2]).numpy().view(np.uint64)
    res = index.search(qc, 300, concepts=[0, 2])
    want = rr.ranked(q, g, 300, mask=mask)
    assert _same((res["idx"], res["dist"]), want)
    idx = want[0]
    bits = np.unpackbits(q.view(np.uint8), axis=1, bitorder="little")[:, None, :] != np.unpackbits(g.view(np.uint8), axis=1, bitorder="little")[idx]
    assert np.array_equal(res["concept_dist"].cpu().numpy(), bits.reshape(Qn, 300, Q, 32).sum(-1))
    assert np.array_equal(res["concept_dist"].cpu().numpy()[:, :, [0, 2]].sum(-1), want[1])
    assert np.array_equal(res["labels"].cpu().numpy(), labels.numpy()[idx]) and res["paths"][3][299] == f"img/{idx[3, 299]}.jpg"
    # deep and within a radius: -1 behind the rows inside it, and the labels / paths / breakdown follow
    r = int(np.median(want[1][:, 150]))
    res = index.search(qc, 300, concepts=[0, 2], radius=r)
    want = rr.ranked(q, g, 300, radius=r, mask=mask)
    assert _same((res["idx"], res["dist"]), want) and (want[0] == -1).any()
    miss = want[0] < 0
    assert (res["labels"].cpu().numpy()[miss] == -1).all() and (res["concept_dist"].cpu().numpy()[miss] == -1).all()
    assert res["paths"][0][299] is None or want[0][0, 299] >= 0
    # k <= 128: without a radius today's call, with one its tail masked
    plain = index.search(qc, 10)
    top = rt.hamming_topk(rt.pack_sign(qc), tg, 10)
    assert torch.equal(plain["idx"], top[0]) and torch.equal(plain["dist"], top[1])
    r = int(np.median(top[1].cpu().numpy()[:, 5]))
    cutres = index.search(qc, 10, radius=r)
    far = top[1] > r
    assert far.any() and not far.all()
    assert torch.equal(cutres["idx"], top[0].masked_fill(far, -1)) and torch.equal(cutres["dist"], top[1].masked_fill(far, -1))
    assert (cutres["labels"][far] == -1).all()
    margin_cut = index.search(qc, 10, margin=0.5, radius=128)          # a per-query mask with a radius: k <= 128 is built
    assert torch.equal(margin_cut["idx"], index.search(qc, 10, margin=0.5)["idx"])
    # what is not built says so
    for kw in (dict(k=129, rank="asymmetric"), dict(k=300, margin=0.5), dict(k=10, rank="asymmetric", radius=3), dict(k=10, radius=-1),
               dict(k=10, radius=129)):
        with pytest.raises(ValueError):
            index.search(qc, **kw)


@pytest.mark.parametrize("labels,remove_first", [("single", False), ("single", True), ("multi", False), ("multi", True)])
def test_evaluate_with_radii_equals_brute_force_and_changes_nothing_else(dev, labels, remove_first):
    from concepthash_amd import retrieval as rt
    nbit, C, Qn, G = 64, 6, 300, 3000
    rng = np.random.default_rng(5)
    centres = rng.integers(0, 2, (1, nbit)).astype(np.uint8) ^ (rng.random((C, nbit)) < 0.15).astype(np.uint8)    # close classes: they overlap
    gl, ql = rng.integers(0, C, G), rng.integers(0, C, Qn)
    g, q = rr.clustered(gl, centres, nbit, 6), rr.clustered(ql, centres, nbit, 7)
    if labels == "multi":
        goh, qoh = np.eye(C, dtype=np.uint8)[gl], np.eye(C, dtype=np.uint8)[ql]
        goh[rng.random(G) < 0.2, 0] = 1
        qoh[rng.random(Qn) < 0.2, 1] = 1
        ql, gl = qoh, goh
    args = (_t(q, dev), _t(g, dev), _t(ql, dev), _t(gl, dev))
    radii = [0, 2, 8]
    ev = rt.evaluate(*args, R=[100, -1], ks=(1, 10), remove_first=remove_first, radii=radii)
    plain = rt.evaluate(*args, R=[100, -1], ks=(1, 10), remove_first=remove_first)
    _, _, d = rr.ranking(q, g)
    want = rr.hash_lookup(d, rr.relevance(ql, gl), radii, remove_first)
    assert np.array_equal(ev["lookup_retrieved"].cpu().numpy(), want["retrieved"])
    assert np.array_equal(ev["lookup_hits"].cpu().numpy(), want["hits"])
    # the case says something: lists with irrelevant rows in them, and queries that retrieve nothing within 0 bits
    assert (want["hits"][:, 2] < want["retrieved"][:, 2]).any() and (want["retrieved"][:, 0] == 0).any() and (want["hits"][:, 2] > 0).any()
    for key, ref in (("precisions_radius", "precisions"), ("recalls_radius", "recalls"), ("retrieved_radius", "retrieved_mean"),
                     ("empty_radius", "empty")):
        assert np.abs(np.asarray(ev[key]) - want[ref]).max() <= 1e-12, key
    assert set(ev) - set(plain) == set(rt.LOOKUP_KEYS)
    for key, v in plain.items():                                        # every other key: the call without radii
        for a, b in zip(v if isinstance(v, list) else [v], ev[key] if isinstance(v, list) else [ev[key]]):
            assert torch.equal(a, b) if torch.is_tensor(a) else a == b, key
    two = rt.evaluate(*args, R=[100, -1], ks=(1, 10), remove_first=remove_first, radii=radii, records=False, tie_bracket=True)
    assert torch.equal(two["lookup_hits"], ev["lookup_hits"]) and two["precisions_radius"] == ev["precisions_radius"]
    empty = rt.evaluate(args[0], args[1][:0], args[2], args[3][:0], radii=radii)
    assert empty["empty_radius"] == [1.0, 1.0, 1.0] and empty["precisions_radius"] == [0.0, 0.0, 0.0]


def test_calculate_map_leaves_the_lookup_in_a_module_attribute(dev):
    from utils import hashing
    rng = np.random.default_rng(9)
    C, nbit = 5, 64
    centres = rng.standard_normal((C, nbit)).astype(np.float32)
    gl, ql = rng.integers(0, C, 800), rng.integers(0, C, 60)
    gc = torch.from_numpy(centres[gl] + 0.8 * rng.standard_normal((800, nbit)).astype(np.float32))
    qc = torch.from_numpy(centres[ql] + 0.8 * rng.standard_normal((60, nbit)).astype(np.float32))
    goh, qoh = torch.eye(C)[gl], torch.eye(C)[ql]
    plain = hashing.calculate_mAP(gc, goh, qc, qoh, -1, PRs=[1, 5])
    assert hashing.last_hash_lookup is None
    out = hashing.calculate_mAP(gc, goh, qc, qoh, -1, PRs=[1, 5], radii=[0, 20])
    look = hashing.last_hash_lookup
    assert out == plain and look["radii"] == [0, 20] and len(look["precisions_radius"]) == 2
    d = ((qc.numpy()[:, None, :] > 0) != (gc.numpy()[None, :, :] > 0)).sum(-1)
    want = rr.hash_lookup(d, rr.relevance(ql, gl), [0, 20])
    for key, ref in (("precisions_radius", "precisions"), ("recalls_radius", "recalls"), ("retrieved_radius", "retrieved_mean"),
                     ("empty_radius", "empty")):
        assert np.abs(np.asarray(look[key]) - want[ref]).max() <= 1e-12, key
    hashing.calculate_mAP(gc, goh, qc, qoh, -1, PRs=[1])
    assert hashing.last_hash_lookup is None
