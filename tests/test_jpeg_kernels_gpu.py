"""The two kernels of the JPEG decode split (csrc/jpeg.hip: `jpeg_idct_kernel`, `jpeg_color_kernel`) pinned on COEFFICIENT BLOCKS:
`ch_jpeg_reconstruct` is driven directly with synthetic descriptors and coefficients -- no file, no entropy decoder -- and must give
the bytes of oracle/jpeg_oracle.py (`reconstruct`: numpy restatement of libjpeg-turbo's islow IDCT, fancy upsampling and YCbCr -> RGB,
itself pinned against Pillow by tests/test_jpeg.py), exactly.  Files an encoder wrote from smooth pictures never reach the clamp branches
of the range limit, most single-coefficient paths of the IDCT, table entries above 255, both clamps of every RGB channel, every width
residue with odd chroma widths, every alignment of an image's output slot or a launch in which workgroups of tiny and wide images and
skipped entries are interleaved; these batches do.  Every block lies inside the domain in which the restated arithmetic is Pillow's
(`jpeg_oracle.in_domain`: what the host decoder lets through), asserted before each launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 0xA5
MODES = {"grey": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}   # ncomp, hs, vs


def _desc(width, height, mode, quant):
    """One live descriptor record; quant [3, 64] (natural order)."""
    from concepthash_amd.jpeg import DESC_DTYPE
    ncomp, hs, vs = MODES[mode]
    d = np.zeros((), dtype=DESC_DTYPE)
    d["width"], d["height"], d["ncomp"], d["hs"], d["vs"] = width, height, ncomp, hs, vs
    d["mcu_w"], d["mcu_h"] = -(-width // (8 * hs)), -(-height // (8 * vs))
    nby, nbc = int(d["mcu_w"]) * hs * int(d["mcu_h"]) * vs, int(d["mcu_w"]) * int(d["mcu_h"])
    d["nblocks"] = nby + 2 * nbc if ncomp == 3 else nby
    d["quant"][:ncomp] = np.asarray(quant)[:ncomp]
    return d


def _dead(width, height, status=11):
    """An entry the host decoder gave up on: a status, no blocks, a slot of its own in the output."""
    from concepthash_amd.jpeg import DESC_DTYPE
    d = np.zeros((), dtype=DESC_DTYPE)
    d["width"], d["height"], d["status"] = width, height, status
    return d


def _counts(d):
    ncomp, hs, vs = int(d["ncomp"]), int(d["hs"]), int(d["vs"])
    nby, nbc = int(d["mcu_w"]) * hs * int(d["mcu_h"]) * vs, int(d["mcu_w"]) * int(d["mcu_h"])
    return [nby] + [nbc, nbc] * (ncomp == 3)


def _fit(coef, quant):
    """coef [n, 64] (any integers), quant [64] -> the blocks scaled, each by the largest factor <= 1 (bisection, 24 steps) that keeps it
    inside the domain: dense blocks AT the domain boundary."""
    from oracle import jpeg_oracle as jo
    coef = np.asarray(coef, dtype=np.float64)
    lo, hi = np.zeros(len(coef)), np.ones(len(coef))
    ok = jo.blocks_in_domain(np.rint(coef).astype(np.int64), quant)
    lo[ok] = 1.0
    for _ in range(24):
        mid = (lo + hi) / 2
        ok = jo.blocks_in_domain(np.rint(coef * mid[:, None]).astype(np.int64), quant)
        lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
    return np.rint(coef * lo[:, None]).astype(np.int16)


def _run(items):
    """items: [(descriptor record, coefficients [nblocks, 64] int16 or None for a dead entry)] -> one `ch_jpeg_reconstruct` launch;
    every live image must equal the oracle byte for byte, every dead entry's slot must still hold the poison.  -> (desc, oracle images)"""
    from concepthash_amd import _lib
    from concepthash_amd.jpeg import GpuJpegDecoder
    from oracle import jpeg_oracle as jo
    lib = _lib.load()
    dev = torch.device("cuda:0")
    desc = np.stack([d for d, _ in items])
    total_coef, total_pix, total_plane = GpuJpegDecoder.layout(desc)
    coef = np.zeros(max(total_coef, 1), np.int16)
    refs = []
    for i, (d, c) in enumerate(items):
        if c is None:
            assert desc["status"][i] != 0 and desc["nblocks"][i] == 0
            refs.append(None)
            continue
        c = np.ascontiguousarray(c, dtype=np.int16)
        assert c.shape == (int(desc["nblocks"][i]), 64), (i, c.shape, int(desc["nblocks"][i]))
        assert jo.in_domain(c, desc[i]), ("a generated block is outside the domain", i)      # checked BEFORE anything is launched
        coef[desc["coef_offset"][i]:desc["coef_offset"][i] + c.size] = c.reshape(-1)
        refs.append(jo.reconstruct(c, desc[i]))
    coef_dev = torch.from_numpy(coef).to(dev)
    desc_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
    planes = torch.full((total_plane + 4096,), POISON, dtype=torch.uint8, device=dev)
    pixels = torch.full((total_pix + 64,), POISON, dtype=torch.uint8, device=dev)
    _lib.check(lib.ch_jpeg_reconstruct(_lib.ptr(coef_dev), _lib.ptr(desc_dev), desc.ctypes.data, len(items), _lib.ptr(planes), _lib.ptr(pixels),
                                       _lib.stream_ptr(torch.cuda.current_stream(dev))), "ch_jpeg_reconstruct")
    torch.cuda.synchronize()
    out = pixels.cpu().numpy()
    assert (out[total_pix:] == POISON).all()                                    # nothing past the last slot
    bad = []
    for i, ref in enumerate(refs):
        h, w, po = int(desc["height"][i]), int(desc["width"][i]), int(desc["pix_offset"][i])
        got = out[po:po + h * w * 3]
        if ref is None:
            assert (got == POISON).all(), ("a skipped entry's slot was written", i)
        elif not np.array_equal(got.reshape(h, w, 3), ref):
            diff = np.argwhere(got.reshape(h, w, 3) != ref)
            bad.append((i, w, h, int(desc["ncomp"][i]), int(desc["hs"][i]), int(desc["vs"][i]), po % 4, len(diff), diff[:3].tolist()))
    assert not bad, (len(bad), bad[:6])
    return desc, refs


def _moderate(rng, d):
    """random coefficients of moderate size for one image: a DC level per block, a sparse decaying AC field"""
    n = int(d["nblocks"])
    u, v = np.mgrid[0:8, 0:8]
    scale = (24.0 / (1 + u + v)).reshape(64)
    c = rng.normal(0, 1, (n, 64)) * scale * (rng.random((n, 64)) < 0.4)
    c[:, 0] = rng.uniform(-60, 60, n)
    out, o = [], 0
    for comp, cnt in enumerate(_counts(d)):
        out.append(_fit(c[o:o + cnt], d["quant"][comp].astype(np.int64)))
        o += cnt
    return np.concatenate(out)


def _tables(rng):
    return np.stack([rng.integers(1, 12, 64), rng.integers(2, 16, 64), rng.integers(3, 20, 64)]).astype(np.uint16)


def test_geometry_batch_every_width_residue_slot_alignment_wide_images_and_skipped_entries():
    """One launch: 13 widths x 5 heights x {grey, 4:4:4, 4:2:2, 4:2:0} shuffled (the output slots then start at every residue mod 4:
    the colour kernel's 32-bit and byte store paths), a 261 x 16 image per mode (more than 256 columns: a second workgroup column of
    the colour kernel; more than 128 blocks: a second workgroup of the IDCT kernel, both beside images whose extra workgroups exit early)
    and skipped entries (status != 0) in front, in the middle and at the back, whose slots must stay untouched."""
    rng = np.random.default_rng(31)
    live = [(w, h, m) for w in (16, 17, 18, 19, 20, 23, 24, 25, 31, 32, 33, 40, 41) for h in (16, 17, 18, 31, 33) for m in MODES]
    live += [(261, 16, m) for m in MODES]
    order = rng.permutation(len(live))
    items = []
    for k in order:
        w, h, m = live[k]
        d = _desc(w, h, m, _tables(rng))
        items.append((d, _moderate(rng, d)))
    items.insert(0, (_dead(21, 17), None))
    items.insert(len(items) // 2, (_dead(35, 19, status=13), None))
    items.append((_dead(18, 23, status=2), None))
    desc, refs = _run(items)
    alive = desc["status"] == 0
    assert set((desc["pix_offset"][alive] % 4).tolist()) == {0, 1, 2, 3}
    assert int(desc["nblocks"].max()) > 128 and int(desc["width"].max()) > 256
    for m, (ncomp, hs, vs) in MODES.items():                                       # every mode has odd and even chroma widths / heights
        sel = alive & (desc["ncomp"] == ncomp) & (desc["hs"] == hs) & (desc["vs"] == vs)
        assert {int(-(-w // hs)) % 2 for w in desc["width"][sel]} == {0, 1} and {int(-(-h // vs)) % 2 for h in desc["height"][sel]} == {0, 1}


def _images_of_blocks(blocks_per_comp, quant, mode, width, height):
    """Pack per-component block lists ([n, 64] each, same n) into images of width x height; short tails are padded with zero blocks."""
    d0 = _desc(width, height, mode, quant)
    per = _counts(d0)[0]
    assert all(c == per for c in _counts(d0))
    n = len(blocks_per_comp[0])
    items = []
    for s in range(0, n, per):
        comps = []
        for b in blocks_per_comp:
            part = np.zeros((per, 64), np.int16)
            part[:len(b[s:s + per])] = b[s:s + per]
            comps.append(part)
        items.append((d0.copy(), np.concatenate(comps)))
    return items


def test_idct_range_limit_every_level_and_every_branch():
    """(a) DC-only blocks with table entry 8: the pass-2 output IS the coefficient, swept over all of [-512, 511] -- every entry of the
    range-limit table, all four branches of `idct_limit` (asserted from the oracle's intermediates).  Grey (the sample is the pixel) and
    4:4:4 (three planes with three different sweeps)."""
    from oracle import jpeg_oracle as jo
    levels = np.arange(-512, 512)
    blocks = np.zeros((1024, 64), np.int16)
    blocks[:, 0] = levels
    q = np.full((3, 64), 8, np.uint16)
    out = jo.idct_stages(blocks, q[0])[2]
    assert np.array_equal(out[:, 0, 0], levels) and (out == out[:, :1, :1]).all()
    assert out.min() == -512 and out.max() == 511
    for lo, hi in ((-512, -129), (-128, -1), (0, 127), (128, 511)):                  # -> 0, x + 128 (twice), 255
        assert ((out >= lo) & (out <= hi)).any()
    rng = np.random.default_rng(3)
    items = _images_of_blocks([blocks], q, "grey", 24, 16) + _images_of_blocks([blocks], q, "grey", 16, 16)
    items += _images_of_blocks([blocks, blocks[rng.permutation(1024)], blocks[::-1]], q, "444", 24, 16)
    _run(items)


def _largest_single(pos, sign):
    """largest |amplitude| of a single coefficient at `pos` (table entry 1) that stays inside the domain"""
    from oracle import jpeg_oracle as jo
    amps = np.arange(1, 4200)
    blocks = np.zeros((len(amps), 64), np.int64)
    blocks[:, pos] = sign * amps
    ok = jo.blocks_in_domain(blocks, np.ones(64, np.int64))
    assert ok[0] and not ok[-1]
    return sign * int(amps[ok].max())


def test_idct_single_coefficients_and_dense_blocks_at_the_domain_boundary():
    """(b) one non-zero coefficient per block: each of the 64 positions, both signs, at the largest amplitude inside the domain, at half
    of it and at the largest amplitude that keeps every sample unclamped -- every term of both passes of `idct_1d` on its own;
    (c) dense random blocks scaled to the domain boundary (outputs reach -512 / 511, the workspace its largest values: where a
    constant that is off by one moves a rounding).  4:4:4 and grey, 16 x 16 and 24 x 16."""
    from oracle import jpeg_oracle as jo
    one = np.ones((3, 64), np.uint16)
    single = []
    for pos in range(64):
        for sign in (1, -1):
            a = _largest_single(pos, sign)
            for amp in (a, a // 2, int(a * 127 / 512)):
                b = np.zeros(64, np.int16)
                b[pos] = amp
                single.append(b)
    single = np.stack(single)
    assert jo.blocks_in_domain(single, one[0]).all()
    rng = np.random.default_rng(17)
    u, v = np.mgrid[0:8, 0:8]
    dense = []
    for k in range(1536):
        shape = [np.ones(64), (1.0 / (1 + u + v)).reshape(64), (1.0 / (1 + u * v)).reshape(64)][k % 3]
        dense.append(rng.normal(0, 3000, 64) * shape * (rng.random(64) < (0.25, 0.6, 1.0)[(k // 3) % 3]))
    dense = np.stack(dense)
    dense[::4, 0] += rng.uniform(-4000, 4000, len(dense[::4]))
    q = np.stack([np.ones(64), rng.integers(1, 6, 64), rng.integers(1, 24, 64)]).astype(np.uint16)
    fitted = [_fit(dense / q[c].astype(np.float64), q[c].astype(np.int64)) for c in range(3)]
    for c in range(3):                                                               # really at the boundary: most blocks reach a limit
        _, ws, out = jo.idct_stages(fitted[c], q[c])
        assert (np.abs(out).reshape(len(out), -1).max(axis=1) >= 500).mean() > 0.7 and np.abs(ws).max() > 12000
    items = _images_of_blocks([single], one, "grey", 16, 16) + _images_of_blocks([single, single[::-1], np.roll(single, 7, 0)], one, "444", 24, 16)
    items += _images_of_blocks([fitted[0]], q, "grey", 24, 16) + _images_of_blocks(fitted, q, "444", 16, 16)
    _run(items)


def test_quant_tables_per_component_and_entries_from_1_to_beyond_255():
    """(d) the kernel multiplies by ITS component's table, read as uint16: tables that differ per component by factors no swap can hide
    (2, 3 and 7 times a common random table), and tables with entries of 1, 255 and 256 ... 2000 (a 16-bit DQT) under coefficients
    small enough for the domain."""
    from oracle import jpeg_oracle as jo
    rng = np.random.default_rng(23)
    items = []
    base = rng.integers(1, 9, 64)
    q = np.stack([2 * base, 3 * base, 7 * base]).astype(np.uint16)
    for w, h in ((16, 16), (24, 16)):
        for _ in range(6):
            d = _desc(w, h, "444", q)
            items.append((d, _moderate(rng, d)))
    big = np.array([1, 255, 256, 300, 511, 1000, 2000], np.int64)
    for k in range(12):
        qq = np.stack([big[rng.integers(0, len(big), 64)] for _ in range(3)]).astype(np.uint16)
        qq[:, 0] = (1, 255, 300)[k % 3]
        mode = ("444", "grey")[k % 2]
        d = _desc(24, 16, mode, qq)
        n = int(d["nblocks"])
        c = np.zeros((n, 64))
        for b in range(n):                                                           # a DC level and two or three small ACs per block
            comp = min(b // _counts(d)[0], 2)
            c[b, 0] = rng.integers(-900, 900) / float(qq[comp, 0])
            for pos in rng.integers(1, 64, 3):
                c[b, pos] = rng.choice([-1, 1]) * max(1, int(400 / float(qq[comp, pos])))
        o, parts = 0, []
        for comp, cnt in enumerate(_counts(d)):
            parts.append(_fit(c[o:o + cnt], qq[comp].astype(np.int64)))
            o += cnt
        c = np.concatenate(parts)
        assert (np.abs(c.reshape(-1, 64)[:, 1:]) > 0).any()
        items.append((d, c))
    desc, _ = _run(items)
    assert int(desc["quant"].max()) > 255 and int(desc["quant"][desc["quant"] > 0].min()) == 1


def test_colour_conversion_both_clamps_of_every_channel():
    """(e) DC-only Y / Cb / Cr blocks (table entry 8: sample = coefficient + 128) at every combination of {0, 64, 128, 192, 255}: the
    corners of the cube drive R, G and B below 0 and above 255 (asserted with the conversion's own formula), the mid values do not."""
    vals = np.array([0, 64, 128, 192, 255])
    Y, Cb, Cr = (a.reshape(-1) for a in np.meshgrid(vals, vals, vals, indexing="ij"))
    cb, cr = Cb.astype(np.int64) - 128, Cr.astype(np.int64) - 128
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), Y + ((116130 * cb + 32768) >> 16)])
    assert (rgb.min(axis=1) < 0).all() and (rgb.max(axis=1) > 255).all() and ((rgb >= 0) & (rgb <= 255)).all(axis=0).any()
    blocks = []
    for plane in (Y, Cb, Cr):
        b = np.zeros((len(plane), 64), np.int16)
        b[:, 0] = plane - 128
        blocks.append(b)
    q = np.full((3, 64), 8, np.uint16)
    _, refs = _run(_images_of_blocks(blocks, q, "444", 16, 16) + _images_of_blocks(blocks, q, "444", 24, 16))
    seen = np.concatenate([r.reshape(-1, 3) for r in refs])
    assert (seen.min(axis=0) == 0).all() and (seen.max(axis=0) == 255).all()


def test_fancy_upsampling_at_the_first_and_last_real_chroma_column_and_row():
    """The triangle filters' edge rules (first / last REAL chroma column: no neighbour outside; first / last real chroma row: the context
    row is the row itself) for odd and even chroma widths and heights, in 4:2:2 and 4:2:0.  Chroma planes are a ramp over the blocks
    (DC-only: a different level per block) with, in the blocks that hold the first and the last real column / row, one high-frequency
    coefficient that makes neighbouring samples differ by tens of levels -- the padding column / row right outside the image included,
    so reading it instead of clamping shows."""
    rng = np.random.default_rng(41)
    items = []
    q = np.stack([np.full(64, 4), np.full(64, 2), np.full(64, 3)]).astype(np.uint16)
    for mode in ("422", "420"):
        _, hs, vs = MODES[mode]
        for w in (17, 18, 19, 20, 31, 32, 33, 34):
            for h in (17, 18, 19, 20, 31, 32, 33):
                d = _desc(w, h, mode, q)
                ny, nc = _counts(d)[0], _counts(d)[1]
                mw, mh = int(d["mcu_w"]), int(d["mcu_h"])
                c = np.zeros((ny + 2 * nc, 64), np.int64)
                c[:ny, 0] = rng.integers(-150, 150, ny)
                dw, dh = -(-w // hs), -(-h // vs)
                for comp in (0, 1):
                    for by in range(mh):
                        for bx in range(mw):
                            blk = c[ny + comp * nc + by * mw + bx]
                            blk[0] = (-200 + 37 * (bx + 2 * by + comp)) // int(q[1 + comp, 0])          # the ramp
                            edge_x = bx in (0, (dw - 1) // 8)
                            edge_y = by in (0, (dh - 1) // 8)
                            if edge_x or edge_y:                     # one coefficient: alternating columns, rows or both
                                pos = (7 if edge_x else 0) + 8 * (7 if edge_y else 0)
                                blk[pos] = rng.choice([-1, 1]) * int(rng.integers(60, 120)) // (1 + (edge_x and edge_y))
                parts = [_fit(c[:ny], q[0].astype(np.int64)), _fit(c[ny:ny + nc], q[1].astype(np.int64)), _fit(c[ny + nc:], q[2].astype(np.int64))]
                items.append((d, np.concatenate(parts)))
    desc, _ = _run(items)
    for hs, vs in ((2, 1), (2, 2)):                                                  # odd and even dw and dh in either sampling
        sel = (desc["hs"] == hs) & (desc["vs"] == vs)
        assert {int(-(-w // hs)) % 2 for w in desc["width"][sel]} == {0, 1}
        assert {int(-(-h // vs)) % 2 for h in desc["height"][sel]} == {0, 1}
