"""GPU: the CLIP text tower of the HIP library (ch_text_*) against the fp32 torch restatement tests/text_tower_ref.py (itself pinned
against transformers in tests/test_text_tower_cpu.py).  Seeded weights built here.  Bounds: DESIGN.md section 2's bf16-encode bounds,
as max-abs (RMS) error over the RMS of the compared tensor -- 2e-2 at two layers, 4e-2 and 1e-2 RMS / RMS at full depth."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import text_tower_ref as ttr

pytestmark = pytest.mark.gpu

# the narrowest width the library accepts: LayerNorm rows and GEMM tiles want dim % 128 == 0, so two heads of 64
SMALL = dict(vocab_size=64, max_position_embeddings=77, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)
LENGTHS = (2, 16, 17, 33, 77)   # inside one key tile, on a tile edge, one past it, across a 32-key block, the CLIP maximum
B = 3


def rel(out, ref):
    """(max-abs error, RMS error) over the RMS of the reference tensor"""
    d = out.detach().cpu().double() - ref.double()
    rms = float(ref.double().pow(2).mean().sqrt())
    return float(d.abs().max()) / rms, float(d.pow(2).mean().sqrt()) / rms


def small_ids(T, seed=0):
    g = torch.Generator().manual_seed(100 * T + seed)
    return torch.randint(0, SMALL["vocab_size"], (B, T), generator=g).numpy().astype(np.int32)


@pytest.fixture(scope="module")
def small():
    from concepthash_amd.text import TextEncoder
    sd = ttr.seeded_text_state_dict(SMALL, seed=1)
    enc = TextEncoder(SMALL, sd, max_batch=B)
    yield enc, sd
    enc.close()


@pytest.fixture(scope="module")
def small_reference(small):
    """T -> (ids, eos, hidden, pooled) of the restatement, computed once"""
    _, sd = small
    out = {}
    for T in LENGTHS:
        ids = small_ids(T)
        eos = np.array([T - 1, T // 2, 0], dtype=np.int32)
        hidden, _ = ttr.text_forward(sd, torch.from_numpy(ids), heads=2)
        out[T] = (ids, eos, hidden, hidden[torch.arange(B), torch.from_numpy(eos).long()])
    return out


@pytest.mark.parametrize("T", LENGTHS)
def test_small_tower_matches_the_restatement(small, small_reference, T):
    enc, _ = small
    ids, eos, ref_hidden, ref_pooled = small_reference[T]
    pooled, hidden = enc.encode_batch(ids, eos, want_hidden=True)
    torch.cuda.synchronize()
    eh, ep = rel(hidden, ref_hidden), rel(pooled, ref_pooled)
    print(f"text tower 128 x 2, T={T}: hidden max-abs/RMS {eh[0]:.3e} (RMS {eh[1]:.3e}), pooled {ep[0]:.3e} ({ep[1]:.3e})")
    assert torch.isfinite(hidden).all() and eh[0] < 2e-2 and ep[0] < 2e-2, (eh, ep)
    # the pooled rows ARE the hidden rows at eos_pos
    assert torch.equal(pooled.cpu(), hidden.cpu()[torch.arange(B), torch.from_numpy(eos).long()])


@pytest.mark.parametrize("T", LENGTHS)
def test_causality_is_bitwise(small, T):
    """Tokens behind position p are replaced by other ids: rows 0..p of out_hidden must not change by one bit (a leak through the
    mask, however small, fails this; so does a row that depends on its neighbours through a GEMM tile)."""
    enc, _ = small
    ids = small_ids(T, seed=1)
    eos = np.zeros(B, dtype=np.int32)
    _, base = enc.encode_batch(ids, eos, want_hidden=True)
    base = base.cpu()
    checked = 0
    for p in sorted({0, 15, 16, T - 2}):
        if p < 0 or p >= T - 1:
            continue
        other = ids.copy()
        other[:, p + 1:] = (other[:, p + 1:] + 1 + np.arange(T - p - 1, dtype=np.int32) % 62) % SMALL["vocab_size"]
        assert (other[:, p + 1:] != ids[:, p + 1:]).all()
        _, got = enc.encode_batch(other, eos, want_hidden=True)
        got = got.cpu()
        assert torch.equal(got[:, :p + 1].view(torch.int32), base[:, :p + 1].view(torch.int32)), (T, p)
        assert not torch.equal(got[:, p + 1], base[:, p + 1])        # ... and the changed tokens did change their own rows
        checked += 1
    assert checked >= 1


def test_padding_id_does_not_matter(small):
    """The same prompts padded with the EOS id and with id 0: out_pooled (first-EOS rows in both) is byte-identical."""
    from concepthash_amd.text import eos_positions
    enc, _ = small
    T, eos_id = 33, 63
    ids = small_ids(T, seed=2) % 62 + 1                                # words in 1..62
    ends = [T - 1, 17, 5]
    for b, e in enumerate(ends):
        ids[b, e] = eos_id
    a, z = ids.copy(), ids.copy()
    for b, e in enumerate(ends):
        a[b, e + 1:] = eos_id
        z[b, e + 1:] = 0
    eos = eos_positions(a, eos_id)
    assert eos.tolist() == ends == eos_positions(z, eos_id).tolist()
    pa, _ = enc.encode_batch(a, eos)
    pz, _ = enc.encode_batch(z, eos)
    assert torch.equal(pa.cpu().view(torch.int32), pz.cpu().view(torch.int32))


def test_argument_checks_return_a_status_and_leave_the_handle_usable(small, small_reference):
    from concepthash_amd import _lib
    enc, _ = small
    lib = enc.lib
    T = 17
    ids, eos, _, ref_pooled = small_reference[T]
    i32p = ctypes.POINTER(ctypes.c_int32)
    out = torch.zeros(B + 1, SMALL["hidden_size"], device=enc.device)

    def call(ids_, eos_, nb):
        ids_, eos_ = np.ascontiguousarray(ids_, dtype=np.int32), np.ascontiguousarray(eos_, dtype=np.int32)
        return lib.ch_text_encode(enc._h, ids_.ctypes.data_as(i32p), eos_.ctypes.data_as(i32p), nb, T, _lib.ptr(out), None, _lib.stream_ptr())

    bad = ids.copy()
    bad[1, 3] = SMALL["vocab_size"]
    assert call(bad, eos, B) != 0 and b"token id 64" in lib.ch_last_error()
    bad[1, 3] = -1
    assert call(bad, eos, B) != 0 and b"token id" in lib.ch_last_error()
    assert call(ids, np.array([0, T, 0]), B) != 0 and b"eos_pos" in lib.ch_last_error()
    assert call(np.concatenate([ids, ids[:1]]), np.concatenate([eos, eos[:1]]), B + 1) != 0 and b"max_batch" in lib.ch_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                               # nothing was launched
    pooled, _ = enc.encode_batch(ids, eos)
    assert rel(pooled, ref_pooled)[0] < 2e-2


@pytest.mark.parametrize("nprompts", [8, 100])
def test_a_real_text_tower_512x12(nprompts):
    """CLIP ViT-B's text tower (512 wide, 8 heads, ffn 2048, 12 layers, quick_gelu), vocabulary cut to 1,000 rows, prompts of 77
    tokens: pooled output inside the full-depth bounds, and every sign that differs from the fp32 restatement belongs to an entry
    whose fp32 magnitude is below the measured max-abs error (the rule of the code-bit test of the image tower).  8 prompts = 616 rows:
    every GEMM runs the 128 x 128 ring kernel.  100 prompts = the codebook's own batch, 7,700 rows: there the dispatcher sends QKV and
    fc1 (186 and 248 tiles of 256 x 256) to the ping-pong kernel -- counted -- and out_proj / fc2 to the ring kernel."""
    from concepthash_amd.text import TextEncoder
    dims = dict(vocab_size=1000, max_position_embeddings=77, hidden_size=512, num_hidden_layers=12, num_attention_heads=8,
                intermediate_size=2048)
    sd = ttr.seeded_text_state_dict(dims, seed=7)
    g = torch.Generator().manual_seed(8)
    ids = torch.randint(0, 999, (nprompts, 77), generator=g)
    for b in range(nprompts):
        ids[b, 76 - 9 * (b % 8):] = 999                                # EOS = the largest id, then padding with it
    enc = TextEncoder(dict(dims, eos_token_id=999), sd, max_batch=nprompts)
    pp_before = int(enc.lib.ch_debug_gemm_dispatch_count(1))
    try:
        pooled, hidden = enc.encode(ids, want_hidden=True)
        torch.cuda.synchronize()
    finally:
        enc.close()
    pp_launches = int(enc.lib.ch_debug_gemm_dispatch_count(1)) - pp_before
    assert pp_launches == (0 if nprompts == 8 else 2 * 12), pp_launches
    ref_hidden, ref_pooled = ttr.text_forward(sd, ids, heads=8, eos_token_id=999)
    ep, eh = rel(pooled, ref_pooled), rel(hidden, ref_hidden)
    err = float((pooled.cpu() - ref_pooled).abs().max())
    flips = pooled.cpu().sign() != ref_pooled.sign()
    print(f"text tower 512 x 12, {nprompts} x 77: pooled max-abs/RMS {ep[0]:.3e} (RMS {ep[1]:.3e}), hidden {eh[0]:.3e} ({eh[1]:.3e}); "
          f"sign flips {int(flips.sum())} of {flips.numel()} ({float(flips.float().mean()):.2e}), max-abs error {err:.3e}")
    assert ep[0] < 4e-2 and ep[1] < 1e-2, ep
    assert eh[0] < 4e-2 and eh[1] < 1e-2, eh
    assert bool((ref_pooled.abs()[flips] < err).all())


def test_end_to_end_codebook_from_a_local_directory(tmp_path, caplog):
    """class_names.txt + a local HF directory -> get_codebook('L') -> (5, dim) of +-1 = sign of the restatement's pooler_output, up to
    entries smaller than the measured error; class_centers with the new keys returns the same tensor and says who built it; without
    class_names.txt it returns the seeded rows."""
    from concepthash_amd.centers import class_centers
    from concepthash_amd.text import ClipBpeTokenizer, TextEncoder
    from trainers.orthohash import class_prompts, get_codebook
    vocab, _ = ttr.synthetic_vocab()
    dims = dict(SMALL, vocab_size=len(vocab))
    sd = ttr.seeded_text_state_dict(dims, seed=9)
    d = str(tmp_path / "clip")
    (tmp_path / "clip").mkdir()
    ttr.write_hf_directory(d, dims, sd)
    names = tmp_path / "class_names.txt"
    names.write_text("001.Black_footed_Albatross\nBrewer's_Blackbird\nwarbler\nthe_bird_of_the_north\nQuail_10\n")
    book = get_codebook("L", 5, 64, class_name_path=str(names), model_id=d, prompt_prefix="a photo of a", quantized=False,
                        binary_method="pca", ae_iters=10000, t=1, identity_scale=1)
    assert tuple(book.shape) == (5, 128) and bool((book.abs() == 1).all())
    ids = ClipBpeTokenizer.from_directory(d)(class_prompts(str(names), "a photo of a "))
    eos_id = vocab["<|endoftext|>"]
    assert ids.shape[0] == 5 and len({int((r == eos_id).argmax()) for r in ids}) > 1          # ragged prompts, padded with EOS
    _, ref_pooled = ttr.text_forward(sd, torch.from_numpy(ids), heads=2, eos_token_id=eos_id)
    enc = TextEncoder(d)
    try:
        pooled = enc.encode(ids).cpu()
    finally:
        enc.close()
    assert rel(pooled, ref_pooled)[0] < 2e-2
    err = float((pooled - ref_pooled).abs().max())
    assert torch.equal(book, pooled.sign())
    diff = book != ref_pooled.sign()
    assert bool((ref_pooled.abs()[diff] < err).all())
    with caplog.at_level(logging.INFO):
        centres = class_centers(5, 128, path=str(tmp_path / "class_centers.pt"), class_name_path=str(names), model_id=d, prompt_prefix="a photo of a ")
    assert torch.equal(centres, book)
    assert any("text tower" in r.getMessage() for r in caplog.records)
    seeded = class_centers(5, 128, path=str(tmp_path / "class_centers.pt"), class_name_path=str(tmp_path / "missing.txt"), model_id=d)
    assert torch.equal(seeded, class_centers(5, 128, path=None)) and not torch.equal(seeded, book)
