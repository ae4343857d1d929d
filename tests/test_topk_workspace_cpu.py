"""CPU: the six ch_*_topk*_workspace functions are host code, so the segment rules behind them -- the list-length table, the residency
rule, the VGPR tables, the plain scan's own rule and "room for the finer of the two segmentations" -- are pinned here without a GPU.

Where the constants come from: they were NOT computed by the code under test.  They are the values the library of commit f07cda5
("Filtered search: top-k among admitted rows only") returned, the parent of the commit that folded the rules into topk_list_index,
topk_per_cu / topk_seg_rows_table and topk_workspace_bytes (csrc/hamming_shared.h); that commit's library returned the same value as
its parent's at every point of Qn in {1, 256, 257, 5794, 100000} x G in {1, 255, 771, 5994, 140001, 1000000, 40000000} x W in 1..4 x
k in {1, 10, 11, 16, 17, 32, 33, 64, 65, 128} for all six functions.  An edit of a table or a rule that moves a segmentation has to
change these numbers on purpose.

One point per (entry, list length) at Qn = 257, G = 140001, W = 2: k = 10, 16, 32, 64, 128 are the longest k of the five lists and
k = 1 the shortest of the first (36 numbers).  At that point two query tiles leave every rule at its 256-row floor, so the six entries
agree; the same 36 at Qn = 5794, G = 1000000, W = 4 are the ones that tell the rules and the tables apart."""
import pytest

KS = (1, 10, 16, 32, 64, 128)
PINNED = {
    (257, 140001, 2): {
        "ch_hamming_topk_workspace": [263184, 2631696, 4210704, 8421392, 16842768, 16842768],
        "ch_hamming_topk_weighted_workspace": [263184, 2631696, 4210704, 8421392, 16842768, 16842768],
        "ch_hamming_topk_filtered_workspace": [263184, 2631696, 4210704, 8421392, 16842768, 16842768],
        "ch_hamming_topk_weighted_filtered_workspace": [263184, 2631696, 4210704, 8421392, 16842768, 16842768],
        "ch_ternary_topk_workspace": [263184, 2631696, 4210704, 8421392, 16842768, 16842768],
        "ch_ternary_topk_filtered_workspace": [263184, 2631696, 4210704, 8421392, 16842768, 16842768],
    },
    (5794, 1000000, 4): {
        "ch_hamming_topk_workspace": [2062680, 20626656, 33002640, 57105680, 48947728, 32631824],
        "ch_hamming_topk_weighted_workspace": [2062680, 20626656, 24473872, 32631824, 32631824, 47464464],
        "ch_hamming_topk_filtered_workspace": [2062680, 20626656, 33002640, 48947728, 48947728, 32631824],
        "ch_hamming_topk_weighted_filtered_workspace": [1784568, 17845536, 24473872, 32631824, 32631824, 47464464],
        "ch_ternary_topk_workspace": [2062680, 20626656, 33002640, 40789776, 48947728, 32631824],
        "ch_ternary_topk_filtered_workspace": [2062680, 20626656, 33002640, 40789776, 48947728, 32631824],
    },
}


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("point", sorted(PINNED))
def test_workspace_sizes_are_the_parent_builds(lib, point):
    Qn, G, W = point
    for entry, want in PINNED[point].items():
        assert [int(getattr(lib, entry)(Qn, G, W, k)) for k in KS] == want, entry


def test_sizes_without_a_segmentation_take_16_bytes(lib):
    """non-positive Qn, G or k: 16 from every entry; W outside 1..4: 16 from every entry but ch_hamming_topk_workspace, which has never
    looked at W (values of the parent build, as above)"""
    for entry in PINNED[(257, 140001, 2)]:
        fn = getattr(lib, entry)
        for Qn, G, k in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5)):
            assert int(fn(Qn, G, 1, k)) == 16, entry
        for W in (0, 5, -3):
            assert int(fn(5, 5, W, 5)) == (5 * 5 * 4 + 16 if entry == "ch_hamming_topk_workspace" else 16), (entry, W)
