"""CPU: the host side of filtered search ("filtered search") -- the numpy reference against a hand-written case,
the bitmap packer, every refusal of `retrieval` and `GalleryIndex.search` that needs no device, the C entries' argument checks, the
groups plane of the index file, and the configuration keys."""
import os

import numpy as np
import pytest
import torch

import filtered_topk_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import build, _lib
    build.build()
    return _lib.load()


# ---- the reference -----------------------------------------------------------------------------------------------------------------

def test_reference_on_a_hand_written_case():
    """12 rows, 2 queries, distances written down by hand; every expected list below was derived on paper"""
    #              row  0  1  2  3  4  5  6  7  8  9 10 11
    D = np.array([[3, 1, 1, 5, 0, 1, 7, 2, 2, 9, 0, 4],
                  [2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]], np.int64)
    allow = np.array([1, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 0], bool)              # rows 2, 4 and 11 are deleted
    group = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], np.int32)
    # no filter: ascending (distance, index)
    idx, dst = ref.topk(D, ref.admitted(2, 12), 4, base=100)
    assert idx.tolist() == [[104, 110, 101, 102], [100, 101, 102, 103]] and dst.tolist() == [[0, 0, 1, 1], [2, 2, 2, 2]]
    # the allow-list alone
    idx, dst = ref.topk(D, ref.admitted(2, 12, allow=allow), 4)
    assert idx.tolist() == [[10, 1, 5, 7], [0, 1, 3, 5]] and dst.tolist() == [[0, 1, 1, 2], [2, 2, 2, 2]]
    # only the query's group; query 1 has none (-1): everything
    adm = ref.admitted(2, 12, group=group, want=[2, -1])
    assert adm[0].tolist() == [False, False, True] * 4 and adm[1].all()
    idx, dst = ref.topk(D, adm, 5)
    assert idx.tolist() == [[2, 5, 8, 11, -1], [0, 1, 2, 3, 4]] and dst.tolist() == [[1, 1, 2, 4, -1], [2, 2, 2, 2, 2]]
    # every group but it, AND the allow-list
    idx, dst = ref.topk(D, ref.admitted(2, 12, allow=allow, group=group, want=[1, 0], exclude=True), 3)
    assert idx.tolist() == [[5, 8, 0], [1, 5, 7]] and dst.tolist() == [[1, 2, 3], [2, 2, 2]]
    # without a plane a row is its own group, numbered from the base: "not the query's own row"
    idx, dst = ref.topk(D, ref.admitted(2, 12, want=[1004, 1000], exclude=True, base=1000), 2, base=1000)
    assert idx.tolist() == [[1010, 1001], [1001, 1002]] and dst.tolist() == [[0, 1], [2, 2]]
    # ... and "only" then leaves that one row; a wanted group nobody has leaves nothing
    idx, dst = ref.topk(D, ref.admitted(2, 12, want=[3, 77]), 2)
    assert idx.tolist() == [[3, -1], [-1, -1]] and dst.tolist() == [[5, -1], [-1, -1]]
    # nothing admitted at all
    idx, dst = ref.topk(D, ref.admitted(2, 12, allow=np.zeros(12, bool)), 3)
    assert (idx == -1).all() and (dst == -1).all()


def test_reference_distances_are_the_existing_references():
    import ternary_ref as tref
    import weighted_topk_ref as wref
    rng = np.random.default_rng(3)
    q = rng.integers(0, 1 << 63, (3, 2), dtype=np.uint64)
    g = rng.integers(0, 1 << 63, (9, 2), dtype=np.uint64)
    m = rng.integers(0, 1 << 63, (2,), dtype=np.uint64)
    pop = lambda a: np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=-1).sum(-1)
    assert np.array_equal(ref.hamming(q, g), pop(q[:, None, :] ^ g[None, :, :]))
    assert np.array_equal(ref.hamming(q, g, m), pop((q[:, None, :] ^ g[None, :, :]) & m))
    w = rng.integers(0, 16, (3, 128)).astype(np.int64)
    assert np.array_equal(ref.weighted(q, g, w), wref.dist(q, g, w))
    tq, tg = rng.integers(-1, 2, (3, 70)).astype(np.int8), rng.integers(-1, 2, (9, 70)).astype(np.int8)
    assert np.array_equal(ref.ternary(tref.planes(tq), tref.planes(tg), 70), tref.dist(tq, tg))


# ---- the bitmap --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 63, 64, 65, 207, 771])
def test_row_bitmap_packs_on_the_cpu(G):
    from concepthash_amd import retrieval as rt
    rng = np.random.default_rng(G)
    allow = rng.random(G) < 0.4
    allow[-1] = True
    bm = rt.row_bitmap(torch.from_numpy(allow))
    assert bm.dtype == torch.int64 and bm.shape == ((G + 63) // 64,) and not bm.is_cuda
    words = bm.numpy().view(np.uint64)
    assert np.array_equal(words, ref.pack_allow(allow))                       # bit r & 63 of word r >> 6, zeros past G
    assert all(((int(words[r >> 6]) >> (r & 63)) & 1) == int(allow[r]) for r in range(G))
    assert rt.bitmap_count(bm, G) == int(allow.sum())
    garbage = torch.from_numpy(ref.pack_allow(allow, garbage=True).view(np.int64))
    assert rt.bitmap_count(garbage, G) == int(allow.sum())                    # what lies past G is ignored
    assert rt.row_bitmap(torch.ones(G, dtype=torch.bool)).numpy().view(np.uint64)[-1] == np.uint64((1 << ((G - 1) % 64 + 1)) - 1)
    with pytest.raises(TypeError):
        rt.row_bitmap(torch.ones(G, dtype=torch.int64))
    with pytest.raises(TypeError):
        rt.row_bitmap(torch.ones(G, 2, dtype=torch.bool))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_retrieval_refuses_bad_filters_before_any_launch():
    from concepthash_amd import retrieval as rt
    Qn, G = 3, 130
    q, g = torch.zeros(Qn, 1, dtype=torch.int64), torch.zeros(G, 1, dtype=torch.int64)
    q3, g3 = torch.zeros(Qn, 2, 1, dtype=torch.int64), torch.zeros(G, 2, 1, dtype=torch.int64)
    ok_allow, ok_group, ok_want = torch.ones(G, dtype=torch.bool), torch.zeros(G, dtype=torch.int32), torch.zeros(Qn, dtype=torch.int64)
    calls = [lambda **kw: rt.hamming_topk_filtered(q, g, 5, **kw), lambda **kw: rt.ternary_topk_filtered(q3, g3, 64, 5, **kw)]
    for call in calls:
        for bad in (torch.ones(G + 1, dtype=torch.bool), torch.ones(G, dtype=torch.int32), torch.ones(2, dtype=torch.int64),
                    torch.ones(4, dtype=torch.int64), torch.ones(G, 1, dtype=torch.bool), [True] * G):
            with pytest.raises(ValueError, match="allow must be"):
                call(allow=bad)
        for bad in (ok_group.long(), ok_group[:-1], ok_group[None, :]):
            with pytest.raises(ValueError, match="group must be"):
                call(group=bad, want=ok_want)
        with pytest.raises(ValueError, match="group without want"):
            call(group=ok_group)
        for bad in (ok_want.int(), ok_want[:-1], torch.zeros(Qn, 1, dtype=torch.int64)):
            with pytest.raises(ValueError, match="want must be"):
                call(want=bad)
        for bad in (1, 0, None, "only"):
            with pytest.raises(TypeError, match="exclude must be a bool"):
                call(allow=ok_allow, exclude=bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):            # a well-formed filter reaches the device check
            call(allow=ok_allow, group=ok_group, want=ok_want, exclude=True)
    with pytest.raises(TypeError):
        rt.hamming_topk_filtered(q.int(), g, 5)
    with pytest.raises(ValueError, match="mask with planes"):
        rt.hamming_topk_filtered(q, g, 5, mask=torch.zeros(1, dtype=torch.int64), planes=torch.zeros(Qn, 4, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="mask must be"):
        rt.hamming_topk_filtered(q, g, 5, mask=torch.zeros(2, dtype=torch.int64))


def _filtered(lib, exclude=0, W=1, k=10, Qn=4, G=4, mask=None, stride=0):
    return lib.ch_hamming_topk_filtered(None, mask, stride, Qn, None, G, W, k, 0, None, None, None, exclude, None, None, None, 0, None)


def test_c_entries_check_their_arguments_on_the_host(lib):
    """the siblings' checks in the siblings' order behind the entry's own name, and exclude in {0, 1}"""
    assert _filtered(lib, W=9) != 0 and b"hamming_topk_filtered: 1 <= W <= 4" in lib.ch_last_error()
    assert _filtered(lib, k=129) != 0 and b"hamming_topk_filtered: 1 <= k <= 128" in lib.ch_last_error()
    assert _filtered(lib, Qn=-1) != 0 and b"negative sizes" in lib.ch_last_error()
    for bad in (2, -1, 7):
        assert _filtered(lib, exclude=bad) != 0 and b"hamming_topk_filtered: exclude must be 0 or 1" in lib.ch_last_error()
    assert _filtered(lib, W=9, exclude=2) != 0 and b"W" in lib.ch_last_error()                   # W first, as ever
    assert _filtered(lib, mask=1, stride=1, W=2) != 0 and b"mask_stride" in lib.ch_last_error()  # a mask: the masked entry's refusal
    assert _filtered(lib) != 0 and b"hamming_topk_filtered: null pointer" in lib.ch_last_error()
    assert _filtered(lib, Qn=0) == 0 and _filtered(lib, Qn=0, exclude=1) == 0
    w = lambda P, exclude=0, k=10: lib.ch_hamming_topk_weighted_filtered(None, None, P, 4, None, 4, 1, k, 0, None, None, None, exclude, None,
                                                                        None, None, 0, None)
    assert w(5) != 0 and b"hamming_topk_weighted_filtered: P" in lib.ch_last_error()
    assert w(8, exclude=3) != 0 and b"hamming_topk_weighted_filtered: exclude must be 0 or 1" in lib.ch_last_error()
    assert w(4, k=0) != 0 and b"hamming_topk_weighted_filtered: 1 <= k <= 128" in lib.ch_last_error()
    t = lambda nbit=64, exclude=0, W=1: lib.ch_ternary_topk_filtered(None, 4, None, 4, W, nbit, 10, 0, None, None, None, exclude, None, None,
                                                                     None, 0, None)
    assert t(exclude=2) != 0 and b"ternary_topk_filtered: exclude must be 0 or 1" in lib.ch_last_error()
    assert t(nbit=65) != 0 and b"nbit" in lib.ch_last_error()
    assert t(W=5) != 0 and b"ternary_topk_filtered: 1 <= W <= 4" in lib.ch_last_error()


def test_filtered_workspaces_cover_the_filtered_segments(lib):
    """at least one list of k keys per query, and never less room than a whole-gallery single segment needs"""
    for name in ("ch_hamming_topk_filtered_workspace", "ch_hamming_topk_weighted_filtered_workspace", "ch_ternary_topk_filtered_workspace"):
        fn = getattr(lib, name)
        assert fn(0, 10, 1, 10) == 16 and fn(10, 0, 1, 10) == 16 and fn(10, 10, 1, 0) == 16
        for Qn, G, W, k in [(1, 1, 1, 1), (70, 207, 1, 10), (257, 771, 4, 128), (256, 140001, 1, 32), (5794, 5994, 2, 32)]:
            assert fn(Qn, G, W, k) >= Qn * k * 4 + 16 and (fn(Qn, G, W, k) - 16) % (Qn * k * 4) == 0


def _index(G=130, labels="single", groups=False):
    from concepthash_amd.search import GalleryIndex
    gen = torch.Generator().manual_seed(5)
    codes = torch.randint(-2 ** 62, 2 ** 62, (G, 1), generator=gen, dtype=torch.int64)
    lab = None
    if labels == "single":
        lab = torch.arange(G) % 5
    elif labels == "rows":
        lab = torch.zeros(G, 5, dtype=torch.uint8)
        lab[torch.arange(G), torch.arange(G) % 5] = 1
        lab[::7, 3] = 1
    return GalleryIndex(codes, 64, 4, labels=lab, groups=(torch.arange(G) % 3).to(torch.int32) if groups else None,
                        real=torch.randn(G, 64, generator=gen))


def test_search_refuses_what_the_scan_does_not_serve():
    """every refusal below comes before anything is launched: the index is on the CPU"""
    ix = _index(groups=True)
    qc = torch.randn(3, 64)
    rows = torch.ones(130, dtype=torch.bool)
    for kw in (dict(rows=rows), dict(labels_in=[1]), dict(labels_out=[1]), dict(query_group=torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(ValueError, match=r"a filter \(\w+\) with rank='cosine' is not built"):
            ix.search(qc, 5, rank="cosine", **kw)
        with pytest.raises(ValueError, match=r"a filter \(\w+\) with k = 129 > 128 is not built"):
            ix.search(qc, 129, **kw)
        with pytest.raises(ValueError, match=r"a filter \(\w+\) with a shortlist is not built"):
            ix.search(qc, 5, rank="dot", shortlist=50, **kw)
    for bad in (torch.ones(129, dtype=torch.bool), torch.ones(130, dtype=torch.int32), torch.ones(4, dtype=torch.int64), [True] * 130):
        with pytest.raises(ValueError, match="rows must be"):
            ix.search(qc, 5, rows=bad)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), [0, 0, 0]):
        with pytest.raises(ValueError, match="query_group must be"):
            ix.search(qc, 5, query_group=bad)
    want = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="group_mode"):
        ix.search(qc, 5, query_group=want, group_mode="not")
    with pytest.raises(ValueError, match="group_by"):
        ix.search(qc, 5, query_group=want, group_by="album")
    with pytest.raises(ValueError, match="groups plane"):
        _index().search(qc, 5, query_group=want)
    for kw in (dict(labels_in=[1]), dict(labels_out=[1])):
        with pytest.raises(ValueError, match="needs the index's labels"):
            _index(labels=None).search(qc, 5, **kw)
    with pytest.raises(ValueError, match="group_by='labels' needs single-label"):
        _index(labels="rows").search(qc, 5, query_group=want, group_by="labels")
    with pytest.raises(ValueError, match="group_by='labels' needs single-label"):
        _index(labels=None).search(qc, 5, query_group=want, group_by="labels")
    with pytest.raises(ValueError, match="outside the index's classes"):
        _index(labels="rows").search(qc, 5, labels_in=[5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # a well-formed filter reaches the device check
        ix.search(qc, 5, rows=rows, labels_in=[1, 2], query_group=want, group_mode="exclude", group_by="row")


def test_search_builds_one_bitmap_from_rows_and_labels():
    from concepthash_amd import retrieval as rt
    G = 130
    rows = torch.arange(G) % 2 == 0
    for kind in ("single", "rows"):
        ix = _index(labels=kind)
        has = lambda c: (ix.labels == c) if kind == "single" else ix.labels[:, c] != 0
        f = ix._filter(3, rows, [1, 3], [3], None, "only", "groups")
        want = rows & (has(1) | has(3)) & ~has(3)
        assert torch.equal(f["allow"], rt.row_bitmap(want)) and f["group"] is None and f["want"] is None and f["exclude"] is False
        packed = torch.from_numpy(ref.pack_allow(rows.numpy(), garbage=True).view(np.int64))
        f = ix._filter(3, packed, None, [0], None, "only", "groups")
        assert rt.bitmap_count(f["allow"], G) == int((rows & ~has(0)).sum())
    ix = _index(groups=True)
    f = ix._filter(3, None, None, None, torch.tensor([0, -1, 2]), "exclude", "groups")
    assert f["allow"] is None and f["group"] is ix.groups and f["exclude"] is True and f["want"].tolist() == [0, -1, 2]
    f = ix._filter(3, None, None, None, torch.tensor([0, -1, 2]), "only", "labels")
    assert f["group"].dtype == torch.int32 and torch.equal(f["group"].long(), ix.labels) and f["exclude"] is False
    assert ix._filter(3, None, None, None, torch.tensor([0, -1, 2]), "exclude", "row")["group"] is None


# ---- the index file ----------------------------------------------------------------------------------------------------------------

def test_groups_plane_survives_save_and_load(tmp_path):
    from concepthash_amd.search import GalleryIndex
    a = _index(groups=True)
    path = str(tmp_path / "index.pth")
    a.save(path)
    raw = torch.load(path, map_location="cpu")
    assert raw["format"] == 1 and raw["groups"].dtype == torch.int32 and torch.equal(raw["groups"], a.groups)
    b = GalleryIndex.load(path)
    assert torch.equal(b.groups, a.groups) and torch.equal(b.to("cpu").groups, a.groups) and torch.equal(b.codes, a.codes)
    # an index without the plane is the file it has always been, and loads as before
    c = _index()
    c.save(path)
    raw = torch.load(path, map_location="cpu")
    assert "groups" not in raw and set(raw) == {"format", "codes", "nbit", "ncontext", "labels", "paths", "data_root", "mean", "transform",
                                                "fingerprint", "real"}
    assert GalleryIndex.load(path).groups is None
    # the plane is checked once, where it is attached
    codes = a.codes
    for bad in (a.groups.long(), a.groups[:-1], a.groups[None, :]):
        with pytest.raises(ValueError, match="groups must be"):
            GalleryIndex(codes, 64, 4, groups=bad)
    neg = a.groups.clone()
    neg[7] = -1
    with pytest.raises(ValueError, match="groups must be >= 0"):
        GalleryIndex(codes, 64, 4, groups=neg)


# ---- configuration -----------------------------------------------------------------------------------------------------------------

def test_search_configuration_takes_the_filter_keys(tmp_path):
    import main_v2
    from concepthash_amd import config as cfglib
    from experiments.search import filter_request
    keys = ("only_classes", "exclude_classes", "exclude_self", "same_class")
    assert all(k in main_v2.SEARCH_KEYS for k in keys)
    base = ["logdir=" + str(tmp_path / "run"), "dataset=synthetic_cub200", "data_dir=" + str(tmp_path)]
    compose = lambda extra: cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", base + extra, cwd=str(tmp_path))
    cfg = compose([])
    assert cfg.only_classes is None and cfg.exclude_classes is None and cfg.exclude_self is False and cfg.same_class is None
    assert all(k in cfg for k in main_v2.SEARCH_KEYS) and filter_request(cfg) is None
    cfg = compose(["only_classes=[3,5]", "exclude_self=true"])
    assert filter_request(cfg) == {"only_classes": [3, 5], "exclude_classes": None, "exclude_self": True, "same_class": None}
    assert filter_request(compose(["same_class=exclude", "exclude_classes=[7]"])) == {"only_classes": None, "exclude_classes": [7],
                                                                                      "exclude_self": False, "same_class": "exclude"}
    with pytest.raises(ValueError, match="same_class"):
        filter_request(compose(["same_class=both"]))
    with pytest.raises(ValueError, match="same_class with exclude_self"):
        filter_request(compose(["same_class=only", "exclude_self=true"]))
    # names are looked up in the dataset's class_names.txt; an unknown one is an error that names the key
    cfg = compose(["only_classes=[Painted Bunting,1]"])
    with pytest.raises(ValueError, match="only_classes.*does not exist"):
        filter_request(cfg)
    folder = os.path.join(str(tmp_path), str(cfg.dataset.data_folder))
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "class_names.txt"), "w") as f:
        f.write("Laysan Albatross\nPainted Bunting\nIndigo Bunting\n")
    assert filter_request(cfg)["only_classes"] == [1, 1]
    with pytest.raises(ValueError, match="exclude_classes: unknown class name 'Dodo'"):
        filter_request(compose(["exclude_classes=[Dodo]"]))
    with pytest.raises(ValueError, match="only_classes: class ids must be >= 0"):
        filter_request(compose(["only_classes=[-2]"]))
