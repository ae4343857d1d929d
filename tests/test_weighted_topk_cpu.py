"""CPU: the host side of the weighted (asymmetric) ranking -- argument validation of ch_weight_planes / ch_hamming_topk_weighted (it runs
before anything touches a GPU), the segment cap of the 16-bit row field, the numpy reference against the real-valued distance it
quantises, and the configuration."""
import ctypes
import os

import numpy as np
import pytest
import torch

import weighted_topk_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from concepthash_amd import build, _lib
    build.build()
    return _lib.load()


X = ctypes.c_void_p(64)      # a non-null pointer that is never read: every case below is refused before a pointer is used


def _planes(lib, codes=X, Qn=4, nbit=64, mask=None, stride=0, P=8, planes=X, wsum=X):
    return lib.ch_weight_planes(codes, Qn, nbit, mask, stride, P, planes, wsum, None)


def _topk(lib, q=X, planes=X, P=8, Qn=4, g=X, G=1000, W=1, k=10, idx=X, dist=X, ws=X, wsb=1 << 40):
    return lib.ch_hamming_topk_weighted(q, planes, P, Qn, g, G, W, k, 0, idx, dist, ws, wsb, None)


def test_weight_planes_refuses_bad_arguments_on_the_host(lib):
    for P in (0, 1, 5, 7, 16, -8):
        assert _planes(lib, P=P) != 0 and b"P (weight bits)" in lib.ch_last_error()
    for nbit in (0, -1, 257, 1 << 20):
        assert _planes(lib, nbit=nbit) != 0 and b"nbit" in lib.ch_last_error()
    for nbit, stride in ((128, 1), (128, 3), (64, 2), (64, -1), (200, 3)):
        assert _planes(lib, nbit=nbit, mask=X, stride=stride) != 0 and b"mask_stride" in lib.ch_last_error()
    assert _planes(lib, Qn=-1) != 0 and b"Qn" in lib.ch_last_error()
    for null in ("codes", "planes", "wsum"):
        assert _planes(lib, **{null: None}) != 0 and b"null pointer" in lib.ch_last_error()
    # both accepted strides pass the checks: with no queries there is nothing to do
    assert _planes(lib, Qn=0, nbit=128, mask=X, stride=0) == 0 and _planes(lib, Qn=0, nbit=128, mask=X, stride=2) == 0
    assert _planes(lib, Qn=0, nbit=256, P=4) == 0


def test_weighted_topk_refuses_bad_arguments_on_the_host(lib):
    for P in (0, 1, 6, 9, 64):
        assert _topk(lib, P=P) != 0 and b"P (weight bits)" in lib.ch_last_error()
    for W in (0, 5, -1):
        assert _topk(lib, W=W) != 0 and b"W" in lib.ch_last_error()
    for k in (0, 129, -3):
        assert _topk(lib, k=k) != 0 and b"k" in lib.ch_last_error()
    assert _topk(lib, Qn=-1) != 0 and b"negative" in lib.ch_last_error()
    assert _topk(lib, G=-1) != 0 and b"negative" in lib.ch_last_error()
    for null in ("q", "planes", "idx", "dist"):
        assert _topk(lib, **{null: None}) != 0 and b"null pointer" in lib.ch_last_error()
    assert _topk(lib, g=None) != 0 and b"null gallery" in lib.ch_last_error()
    need = lib.ch_hamming_topk_weighted_workspace(4, 1000, 1, 10)
    assert need >= 4 * 4 * 10 + 16
    assert _topk(lib, wsb=need - 1) != 0 and b"workspace too small" in lib.ch_last_error()
    assert _topk(lib, ws=None) != 0 and b"workspace too small" in lib.ch_last_error()
    # 65,536 rows per segment at the most (16-bit row field), 65,535 segments (grid.y): one more row is one segment too many
    assert _topk(lib, Qn=1, G=65536 * 65535 + 1, k=1) != 0 and b"65,535 segments" in lib.ch_last_error()
    assert _topk(lib, Qn=0) == 0                                   # no queries: nothing to do, as ch_hamming_topk
    assert lib.ch_hamming_topk_weighted_workspace(0, 1000, 1, 10) == 16 == lib.ch_hamming_topk_weighted_workspace(4, 0, 1, 10)


def test_weighted_topk_segments_hold_at_most_65536_rows(lib):
    """key = D << 16 | row-in-segment: whatever the chip-fill rule wants, a segment is cut at 2^16 rows.  The workspace is one uint32
    list of k keys per (segment, query) + 16 bytes, so it shows the segment count."""
    Qn, G, k = 200_000, 80_000_000, 10
    nbytes = lib.ch_hamming_topk_weighted_workspace(Qn, G, 1, k)
    assert (nbytes - 16) % (4 * Qn * k) == 0
    assert (nbytes - 16) // (4 * Qn * k) >= -(-G // 65536) == 1221
    # ... and the unweighted scan, with 23 bits of row, keeps its own (coarser) segmentation
    assert (lib.ch_hamming_topk_workspace(Qn, G, 1, k) - 16) // (4 * Qn * k) < 1221


@pytest.mark.parametrize("nbit", [48, 64, 120, 256])
@pytest.mark.parametrize("bits", [4, 8])
def test_reference_distance_is_the_rounded_real_valued_distance(nbit, bits):
    """D / L * amax against (sum |c| - c . s) / 2 = the sum of |c_j| over the disagreeing bits: every weight is off by at most half a
    quantisation step amax / L, so the two differ by at most nbit amax / (2 L)"""
    rng = np.random.default_rng(nbit + bits)
    Qn, G, L = 33, 57, (1 << bits) - 1
    c = rng.standard_normal((Qn, nbit)).astype(np.float32)
    gal = rng.standard_normal((G, nbit)).astype(np.float32)
    w = ref.weights(c, bits)
    assert w.shape == (Qn, 64 * ((nbit + 63) // 64)) and w.min() == 0 and w.max() == L and (w[:, nbit:] == 0).all()
    D = ref.dist(ref.pack_sign(c), ref.pack_sign(gal), w)
    assert (D >= 0).all() and (D <= w.sum(1)[:, None]).all()
    c64 = c.astype(np.float64)
    s = np.where(gal > 0, 1.0, -1.0)                                    # the +-1 gallery code
    exact = (np.abs(c64).sum(1)[:, None] - c64 @ s.T) / 2
    amax = np.abs(c64).max(1)[:, None]
    err = np.abs(D / L * amax - exact)
    assert (err <= nbit * amax / (2 * L) * (1 + 1e-12)).all(), float((err / (nbit * amax / (2 * L))).max())
    # planes are the bits of the weights, and the plane form of D is the same integer
    planes = ref.planes_of(w, bits)
    assert planes.shape == (Qn, bits, w.shape[1] // 64) and planes.dtype == np.uint64
    x = ref.pack_sign(c)[:, None, None, :] ^ ref.pack_sign(gal)[None, :, None, :]                    # [Qn, G, 1, W]
    pop = ref.bits_of(x & planes[:, None, :, :]).sum(-1, dtype=np.int64)                              # [Qn, G, P]
    assert np.array_equal((pop << np.arange(bits)).sum(-1), D)


def test_reference_rounding_mask_and_non_finite_values():
    c = np.zeros((4, 64), np.float32)
    c[0, :5] = [255.0, 0.5, 1.5, 126.5, -254.5]                        # a / amax = (m + 0.5) / L exactly: rounds up
    c[1, :4] = [np.nan, np.inf, -np.inf, 2.0]
    c[3, :3] = [1.0, -3.0, 0.5]
    w = ref.weights(c, 8)
    assert w[0, :5].tolist() == [255, 1, 2, 127, 255] and w[1, :4].tolist() == [0, 0, 0, 255] and not w[2].any()
    assert w[3, :3].tolist() == [85, 255, 43]                          # 0.5 * 255 / 3 = 42.5 -> 43
    mask = np.array([0b101], dtype=np.uint64)                          # bit 1 (the row's maximum) masked out: amax is 1.0
    assert ref.weights(c, 8, mask)[3, :3].tolist() == [255, 0, 128] and ref.weights(c, 4, mask)[3, :3].tolist() == [15, 0, 8]
    per = np.array([[0xFF], [0x7], [0xFF], [0]], dtype=np.uint64)
    w = ref.weights(c, 8, per)
    assert not w[1].any() and not w[3].any() and w[0, :5].tolist() == [255, 1, 2, 127, 255]
    idx, dst = ref.topk(np.array([[5, 1, 5, 1, 0]]), 7, base=100)
    assert idx.tolist() == [[104, 101, 103, 100, 102, -1, -1]] and dst.tolist() == [[0, 1, 1, 5, 5, -1, -1]]


def test_search_configuration_takes_rank_and_weight_bits(tmp_path):
    import main_v2
    from concepthash_amd import config as cfglib
    base = ["logdir=" + str(tmp_path / "run"), "dataset=synthetic_cub200"]
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", base + ["rank=asymmetric", "weight_bits=4"], cwd=str(tmp_path))
    assert cfg.rank == "asymmetric" and cfg.weight_bits == 4
    assert "rank" in main_v2.SEARCH_KEYS and "weight_bits" in main_v2.SEARCH_KEYS and all(k in cfg for k in main_v2.SEARCH_KEYS)
    cfg = cfglib.compose(os.path.join(ROOT, "configs"), "search.yaml", base, cwd=str(tmp_path))
    assert cfg.rank == "hamming" and cfg.weight_bits == 8                          # the defaults: today's ranking


def test_gallery_index_refuses_an_unknown_rank_before_any_library_call(monkeypatch):
    from concepthash_amd import _lib
    from concepthash_amd.search import GalleryIndex

    def no_library():
        raise AssertionError("the library was loaded before the rank was checked")
    monkeypatch.setattr(_lib, "load", no_library)
    index = GalleryIndex(torch.zeros(5, 1, dtype=torch.int64), 64, 4)               # a CPU index
    with pytest.raises(ValueError, match="rank"):
        index.search(torch.randn(3, 64), 2, rank="nearest")
    with pytest.raises(ValueError, match="weight_bits"):
        index.search(torch.randn(3, 64), 2, rank="asymmetric", weight_bits=5)
