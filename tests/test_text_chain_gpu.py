"""GPU: the CLIP text tower (csrc/text_model.hip), kernel by kernel and as a chain.

(a) text_embed_kernel alone through ch_debug_text_embed, bit for bit; (b) text_pool_kernel alone through ch_debug_text_pool, inside the
bound derived in tests/text_chain_ref.py, eos mode bit-identical to the same rows of the all-rows launch; (c) the whole chain REBUILT from
the taps -- embed, then per layer ch_debug_layernorm_f32, ch_debug_gemm_fwd (every GemmParams field as run_text fills it),
ch_debug_attention_causal, ..., then pool -- with every stage held, on the GPU's own input to that stage, to the Hugging Face definition
of that stage (text_chain_ref.compose) within the bound its launcher already has; (d) ch_text_encode equal to that composition BIT FOR
BIT, so that (c) and (d) together pin the product chain per stage to about a bf16 half ulp; (e) handle state: shorter after longer calls,
back-to-back calls through the pinned staging buffer with the caller's arrays overwritten, a non-default stream, exactly sized outputs.

Launch discipline of tests/kernel_launch.py: outputs between sentinel guard blocks and themselves the sentinel, NaN behind every float
input, a second identical launch with identical bytes, the worst error / bound ratio of every group printed (-s).  Ids and eos
positions are always in range; nothing is tuned to a measured error and nothing is run repeatedly to look for a difference.

Worst error / bound ratios measured on an MI355X (1.0 is the bound; observations, not limits; no stage breached one, every bitwise
assertion held, no kernel was changed):
  text_pool 0.554, eos mode 0.605 (text_embed bit-exact)
  chain A (128 wide, T = 1 .. 288): ln 1.000, gemm 0.988, attn 0.670, resid 0.017, pool 0.146      B (gelu, eps 1e-6): 1.000, 0.987, 0.662, 0.012, 0.140
  chain C (384 wide, six heads): 0.999, 0.957, 0.632, 0.004, 0.124                                 D (1280 wide): 0.999, 0.979, 0.694, 0.006, 0.080
A bf16 output sits at 1.000 where the fp32 value falls on a rounding tie (error = the half ulp that IS the bound).
"""
import ctypes

import numpy as np
import pytest
import torch

import text_chain_ref as tc
import text_tower_ref as ttr
import train_kernels_ref as tr
from kernel_launch import Out, inp, report, twice, within

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAST = 3                                  # sentinel rows behind a single kernel's output
I32P = ctypes.POINTER(ctypes.c_int32)

# name -> (dim, heads, ffn, layers, max_positions, act, eps, B, lengths)
CASES = {
    "A": (128, 2, 256, 2, 288, "quick_gelu", 1e-5, 3, (1, 17, 77, 129, 288)),     # the KB = 1, 3, 5 and 9 causal instances
    "B": (128, 2, 256, 1, 288, "gelu", 1e-6, 3, (17, 77)),                        # exact gelu and a non-default eps
    "C": (384, 6, 384, 1, 77, "quick_gelu", 1e-5, 2, (33,)),                      # width 384, six heads
    "D": (1280, 20, 256, 1, 16, "quick_gelu", 1e-5, 2, (5,)),                     # the MAXP edge of the row kernels
}
CASE_T = [(name, T) for name, c in CASES.items() for T in c[8]]
BIG = (512, 8, 2048, 2, 77, "quick_gelu", 1e-5, 100, (77,))                       # 7,700 rows: QKV and fc1 on the 256x256 ping-pong kernel
BIG_VOCAB = 1000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from concepthash_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """a HIP error (an illegal access, say) ends the session: nothing more is launched on a device that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after a test, nothing more is launched: {e}", returncode=3)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- (a) text_embed_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", tc.EMBED_D)
def test_text_embed_is_exact(dev, L, D):
    lib = L.load()
    for B, T in tc.EMBED_BT:
        rows = B * T
        ids, tok, pos = tc.embed_inputs(B, T, D)
        want = tc.embed_ref(ids, T, tok, pos)
        idd, tokd, posd = ids.to(dev), inp(dev, tok), inp(dev, pos)

        def launch():
            out = Out(dev, (rows + PAST, D), F32)
            L.check(lib.ch_debug_text_embed(L.ptr(idd), rows, T, D, L.ptr(tokd), L.ptr(posd), out.ptr, L.stream_ptr()), "text_embed")
            return [out]

        out = twice(launch)[0]
        assert tr.bits_equal(out.get()[:rows].contiguous(), want), f"text_embed {B}x{T} D {D}"
        behind = torch.zeros(rows + PAST, D, dtype=torch.bool)
        behind[rows:] = True
        assert out.untouched(behind), f"text_embed {B}x{T} D {D}: rows behind the output were written"
    for bad in (D + 64, 1408):
        assert lib.ch_debug_text_embed(L.ptr(idd), 1, 1, bad, L.ptr(tokd), L.ptr(posd), L.ptr(torch.zeros(4, device=dev)), L.stream_ptr()) != 0
        assert b"text_embed" in lib.ch_last_error()


# ---- (b) text_pool_kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", tc.POOL_D)
def test_text_pool_within_its_bound(dev, L, D):
    lib = L.load()
    w, b = tc.fr.affine_params(D, "final")
    wd, bd = inp(dev, w), inp(dev, b)

    def run(Hd, eos_d, nrows, T, eps):
        def launch():
            out = Out(dev, (nrows + PAST, D), F32)
            L.check(lib.ch_debug_text_pool(L.ptr(Hd), L.ptr(eos_d), nrows, T, D, L.ptr(wd), L.ptr(bd), eps, out.ptr, L.stream_ptr()), "text_pool")
            return [out]
        out = twice(launch)[0]
        behind = torch.zeros(nrows + PAST, D, dtype=torch.bool)
        behind[nrows:] = True
        assert out.untouched(behind), "text_pool: rows behind the output were written"
        return out.get()[:nrows].contiguous()

    for eps in tc.POOL_EPS:
        for fam in tc.ROW_FAMILIES:
            for rows in tc.POOL_ROWS:
                H = tc.row_family(fam, rows, D, "pool")
                ref, bound = tc.pool_ref(H, None, 1, w, b, eps)
                within("text_pool", run(inp(dev, H), None, rows, 1, eps), ref, bound, f"{fam} {rows}x{D} eps {eps}")
            for B, T, eos in tc.POOL_EOS:
                H = tc.row_family(fam, B * T, D, "pool_eos")
                e = torch.tensor(eos, dtype=torch.int32)
                Hd = inp(dev, H)
                ref, bound = tc.pool_ref(H, e, T, w, b, eps)
                got = run(Hd, e.to(dev), B, T, eps)
                within("text_pool eos", got, ref, bound, f"{fam} eos {B}x{T} D {D} eps {eps}")
                full = run(Hd, None, B * T, T, eps)
                assert tr.bits_equal(got, full[torch.arange(B) * T + e.long()].contiguous()), f"{fam} eos {B}x{T} D {D}: not the all-rows launch's rows"
    report("text_pool", "text_pool eos")
    Hd = inp(dev, tc.row_family("benign", 1, D, "pool"))
    for bad in (D + 64, 1408):
        assert lib.ch_debug_text_pool(L.ptr(Hd), None, 1, 1, bad, L.ptr(wd), L.ptr(bd), 1e-5, L.ptr(torch.zeros(4, device=dev)), L.stream_ptr()) != 0
        assert b"text_pool" in lib.ch_last_error()


# ---- (c) the chain rebuilt from the taps ---------------------------------------------------------------------------------------------------
def _dims(case, vocab=tc.VOCAB):
    D, heads, ffn, layers, maxpos = case[:5]
    return dict(vocab_size=vocab, max_position_embeddings=maxpos, hidden_size=D, num_hidden_layers=layers, num_attention_heads=heads,
                intermediate_size=ffn, hidden_act=case[5], layer_norm_eps=case[6])


def _ids(B, T, vocab, seed=0):
    return torch.randint(0, vocab, (B, T), generator=tc.gen("ids", B, T, vocab, seed)).numpy().astype(np.int32)


def _eos(B, T):
    return np.array([T - 1, T // 2, 0] * (B // 3 + 1), dtype=np.int32)[:B].copy()


class Composition:
    """The text chain made of the taps, on buffers of the handle's padded row count (zero-filled), every tap argument filled as run_text
    fills its launch: weights converted as the loader converts them (fp32 tables; bf16, round to nearest even, for the four GEMM weights,
    q | k | v stacked -- ch_convert_bf16 is pinned bit-exact in tests/test_forward_kernels_gpu.py)."""

    def __init__(self, L, dev, case, sd, vocab=tc.VOCAB):
        self.L, self.lib, self.dev = L, L.load(), dev
        self.D, self.heads, self.ffn, self.layers, self.maxpos, self.act, self.eps, self.max_batch = case[:8]
        D, M = self.D, self.ffn
        self.rows_alloc = (self.max_batch * self.maxpos + 255) // 256 * 256 + 256
        g = lambda k: sd[tc.TM + k].detach().to(F32)   # noqa: E731
        self.tok, self.pos = inp(dev, g("embeddings.token_embedding.weight")), inp(dev, g("embeddings.position_embedding.weight"))
        self.fln = (g("final_layer_norm.weight"), g("final_layer_norm.bias"))
        self.fln_d = tuple(inp(dev, t) for t in self.fln)
        self.w = [tc.layer_weights(sd, i) for i in range(self.layers)]
        self.wd = [{k: inp(dev, v) for k, v in w.items()} for w in self.w]
        z = lambda cols, dt: torch.zeros(self.rows_alloc, cols, dtype=dt, device=dev)   # noqa: E731
        self.H, self.Xn, self.QKV, self.AO, self.A, self.F1 = z(D, F32), z(D, BF16), z(3 * D, BF16), z(D, BF16), z(D, BF16), z(M, BF16)

    def _gemm(self, rows, X, W, bias, N, K, epi, out, ldo):
        L = self.L
        # resid = H, ldr = D on every GEMM, X_rows_alloc = the padded row count, variant 0 and no option set: GemmParams as run_text's lambda fills it
        L.check(self.lib.ch_debug_gemm_fwd(0, L.ptr(X), self.rows_alloc, L.ptr(W), L.ptr(bias), rows, N, K, epi, L.ptr(out), ldo, L.ptr(self.H), self.D,
                                           None, None, 0, None, None, 0.0, None, None, 0, 0, 0, 0, 0, 0, L.stream_ptr()), "gemm_fwd")

    def run(self, ids, eos, check=None):
        """ids [B, T], eos [B] (numpy int32) -> (pooled Out [B, D], hidden Out [B * T, D]); check(stage, layer, x, h, got): called after each
        stage with CPU copies of its input, of the residual stream before it (residual stages) and of its output"""
        L, lib, dev = self.L, self.lib, self.dev
        B, T = ids.shape
        rows, D, M = B * T, self.D, self.ffn
        idd, eosd = torch.from_numpy(ids.reshape(-1).copy()).to(dev), torch.from_numpy(eos.copy()).to(dev)
        s = L.stream_ptr

        def seen(stage, layer, x, h, got, cols):
            if check is not None:
                torch.cuda.synchronize()
                check(stage, layer, x[:rows].cpu(), None if h is None else h[:rows].cpu(), got[:rows, :cols].cpu())

        L.check(lib.ch_debug_text_embed(L.ptr(idd), rows, T, D, L.ptr(self.tok), L.ptr(self.pos), L.ptr(self.H), s()), "text_embed")
        if check is not None:
            torch.cuda.synchronize()
            check("embed", -1, torch.from_numpy(ids.reshape(-1).copy()), None, self.H[:rows].cpu())
        act_epi = tc.ACT_EPI[self.act]
        for i, w in enumerate(self.wd):
            ln = lambda a, b: L.check(lib.ch_debug_layernorm_f32(L.ptr(self.H), rows, D, L.ptr(a), L.ptr(b), self.eps, L.ptr(self.Xn), s()), "layernorm_f32")   # noqa: E731
            ln(w["ln1_w"], w["ln1_b"])
            seen("ln1", i, self.H, None, self.Xn, D)
            self._gemm(rows, self.Xn, w["qkv_w"], w["qkv_b"], 3 * D, D, tc.gr.EPI_BIAS, self.QKV, 3 * D)
            seen("qkv", i, self.Xn, None, self.QKV, 3 * D)
            L.check(lib.ch_debug_attention_causal(L.ptr(self.QKV), B, T, self.heads, L.ptr(self.AO), s()), "attention_causal")
            seen("attn", i, self.QKV, None, self.AO, D)
            h0 = self.H.clone() if check is not None else None
            self._gemm(rows, self.AO, w["out_w"], w["out_b"], D, D, tc.gr.EPI_BIAS_RESID, self.A, D)
            seen("out_proj", i, self.AO, h0, self.H, D)
            seen("out_proj_copy", i, self.AO, h0, self.A, D)
            ln(w["ln2_w"], w["ln2_b"])
            seen("ln2", i, self.H, None, self.Xn, D)
            self._gemm(rows, self.Xn, w["fc1_w"], w["fc1_b"], M, D, act_epi, self.F1, M)
            seen("fc1", i, self.Xn, None, self.F1, M)
            h0 = self.H.clone() if check is not None else None
            self._gemm(rows, self.F1, w["fc2_w"], w["fc2_b"], D, M, tc.gr.EPI_BIAS_RESID, self.A, D)
            seen("fc2", i, self.F1, h0, self.H, D)
            seen("fc2_copy", i, self.F1, h0, self.A, D)
        pooled, hidden = Out(dev, (B, D), F32), Out(dev, (rows, D), F32)
        L.check(lib.ch_debug_text_pool(L.ptr(self.H), L.ptr(eosd), B, T, D, L.ptr(self.fln_d[0]), L.ptr(self.fln_d[1]), self.eps, pooled.ptr, s()), "text_pool")
        L.check(lib.ch_debug_text_pool(L.ptr(self.H), None, rows, T, D, L.ptr(self.fln_d[0]), L.ptr(self.fln_d[1]), self.eps, hidden.ptr, s()), "text_pool")
        torch.cuda.synchronize()
        if check is not None:
            check("pool", -1, self.H[:rows].cpu(), None, (pooled.get(), hidden.get(), torch.from_numpy(eos.copy())))
        # nothing wrote behind the call's rows: the padding rows are still the zeros they were
        for buf in (self.H, self.Xn, self.QKV, self.AO, self.A, self.F1):
            assert not bool(buf[self.max_batch * self.maxpos:].view(torch.int16 if buf.dtype == BF16 else torch.int32).any()), "a padding row was written"
        return pooled, hidden


@pytest.fixture(scope="module")
def towers(L, dev):
    """case name -> (case, state dict, Composition, TextEncoder): built once, closed at the end"""
    from concepthash_amd.text import TextEncoder
    made = {}
    for k, (name, case) in enumerate(CASES.items()):
        sd = ttr.seeded_text_state_dict(_dims(case), seed=11 + k)
        made[name] = (case, sd, Composition(L, dev, case, sd), TextEncoder(_dims(case), sd, max_batch=case[7]))
    yield made
    for _, _, _, enc in made.values():
        enc.close()


@pytest.fixture(scope="module")
def composed():
    """(case name, T) -> (ids, eos, pooled bits, hidden bits) of the composition, filled by the stage test and read by the equality test"""
    return {}


def _compose_run(towers, composed, name, T, check=None):
    case, _, comp, _ = towers[name]
    B = case[7]
    ids, eos = _ids(B, T, tc.VOCAB), _eos(B, T)
    pooled, hidden = comp.run(ids, eos, check)
    composed[(name, T)] = (ids, eos, pooled.raw().clone(), hidden.raw().clone())
    return composed[(name, T)]


@pytest.mark.parametrize("name,T", CASE_T)
def test_every_stage_of_the_composed_chain_within_its_bound(towers, composed, name, T):
    case, sd, comp, _ = towers[name]
    D, heads, _, _, _, act, eps, B, _ = case
    grp = f"text chain {name}"

    def check(stage, layer, x, h, got):
        what = f"{stage} layer {layer} T {T}"
        if stage == "embed":
            want = tc.embed_ref(x, T, sd[tc.TM + "embeddings.token_embedding.weight"].float(), sd[tc.TM + "embeddings.position_embedding.weight"].float())
            assert tr.bits_equal(got, want), f"{grp} {what}"
        elif stage == "pool":
            pooled, hidden, eos = got
            ref, bound = tc.pool_ref(x, None, T, comp.fln[0], comp.fln[1], eps)
            within(grp + " pool", hidden, ref, bound, what)
            ref, bound = tc.pool_ref(x, eos, T, comp.fln[0], comp.fln[1], eps)
            within(grp + " pool", pooled, ref, bound, what + " eos")
            assert tr.bits_equal(pooled, hidden[torch.arange(B) * T + eos.long()].contiguous()), f"{grp} {what}: pooled rows are not the hidden rows"
        else:
            want, bound = tc.compose(stage, comp.w[layer], x, B, T, heads, act, eps, h=h)
            kind = "ln" if stage in ("ln1", "ln2") else "attn" if stage == "attn" else "resid" if stage in ("out_proj", "fc2") else "gemm"
            within(f"{grp} {kind}", got, want, bound, what)

    _compose_run(towers, composed, name, T, check)
    report(*(f"{grp} {k}" for k in ("ln", "gemm", "attn", "resid", "pool")))


# ---- (d) the product chain equals the composition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", CASE_T)
def test_the_product_chain_is_the_composition_bit_for_bit(towers, composed, name, T):
    enc = towers[name][3]
    ids, eos, pooled_bits, hidden_bits = composed.get((name, T)) or _compose_run(towers, composed, name, T)
    pooled, hidden = enc.encode_batch(ids, eos, want_hidden=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(hidden).view(hidden_bits.shape), hidden_bits), f"case {name} T {T}: last_hidden_state differs from the composition"
    assert torch.equal(_bits(pooled), pooled_bits), f"case {name} T {T}: pooler_output differs from the composition"


def test_the_product_chain_is_the_composition_at_7700_rows(L, dev):
    """B = 100, T = 77 on a 512-wide, two-layer tower: the dispatcher sends QKV and fc1 to the 256x256 ping-pong kernel, in the product call
    and in the composition alike (counted); bytes only, no fp64 reference"""
    from concepthash_amd.text import TextEncoder
    lib = L.load()
    sd = ttr.seeded_text_state_dict(_dims(BIG, BIG_VOCAB), seed=21)
    B, T = BIG[7], BIG[8][0]
    ids, eos = _ids(B, T, BIG_VOCAB), _eos(B, T)
    n0 = int(lib.ch_debug_gemm_dispatch_count(1))
    pooled, hidden = Composition(L, dev, BIG, sd, BIG_VOCAB).run(ids, eos)
    n1 = int(lib.ch_debug_gemm_dispatch_count(1))
    enc = TextEncoder(_dims(BIG, BIG_VOCAB), sd, max_batch=B)
    try:
        p, h = enc.encode_batch(ids, eos, want_hidden=True)
        torch.cuda.synchronize()
    finally:
        enc.close()
    n2 = int(lib.ch_debug_gemm_dispatch_count(1))
    assert n1 - n0 == n2 - n1 and n1 - n0 != 0, (n1 - n0, n2 - n1)
    assert n1 - n0 == 2 * BIG[3]                                             # QKV and fc1 of each layer
    assert torch.equal(_bits(h).view(B * T, -1), hidden.raw()) and torch.equal(_bits(p), pooled.raw())


# ---- (e) handle state: the public entry points only, on case A's dimensions with max_batch = 3 ---------------------------------------------
@pytest.fixture()
def fresh_a(towers):
    """a factory of new handles of case A (closed after the test)"""
    from concepthash_amd.text import TextEncoder
    case, sd = towers["A"][:2]
    made = []

    def make():
        made.append(TextEncoder(_dims(case), sd, max_batch=case[7]))
        return made[-1]
    yield make
    for enc in made:
        enc.close()


def _call(enc, ids, eos):
    p, h = enc.encode_batch(ids, eos, want_hidden=True)
    torch.cuda.synchronize()
    return _bits(p), _bits(h)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_shorter_call_after_a_longer_one_and_the_other_way_round(fresh_a):
    small, large = (_ids(1, 2, tc.VOCAB, 1), _eos(1, 2)), (_ids(3, 288, tc.VOCAB, 1), _eos(3, 288))
    alone_small, alone_large = _call(fresh_a(), *small), _call(fresh_a(), *large)
    enc = fresh_a()
    assert _same(_call(enc, *large), alone_large)
    assert _same(_call(enc, *small), alone_small), "(1, 2) after (3, 288) is not (1, 2) on a fresh handle"
    enc = fresh_a()
    assert _same(_call(enc, *small), alone_small)
    assert _same(_call(enc, *large), alone_large), "(3, 288) after (1, 2) is not (3, 288) on a fresh handle"


def test_two_calls_in_a_row_through_the_staging_buffer(fresh_a):
    """no host synchronisation between the calls; the caller's arrays are overwritten with other valid ids as soon as each call returns"""
    B, T = 3, 77
    first, second, other = (_ids(B, T, tc.VOCAB, s) for s in (2, 3, 4))
    eos1, eos2 = _eos(B, T), np.array([5, 0, T - 1], dtype=np.int32)
    alone1, alone2 = _call(fresh_a(), first, eos1), _call(fresh_a(), second, eos2)
    enc = fresh_a()
    a_ids, a_eos = first.copy(), eos1.copy()
    p1, h1 = enc.encode_batch(a_ids, a_eos, want_hidden=True)
    a_ids[:], a_eos[:] = other, 1
    b_ids, b_eos = second.copy(), eos2.copy()
    p2, h2 = enc.encode_batch(b_ids, b_eos, want_hidden=True)
    b_ids[:], b_eos[:] = other, 2
    torch.cuda.synchronize()
    assert _same((_bits(p1), _bits(h1)), alone1), "the first call read its arrays after it returned, or the second overwrote its staging"
    assert _same((_bits(p2), _bits(h2)), alone2), "the second call is not that call made alone"


def test_a_side_stream_gives_the_default_streams_bytes(fresh_a, dev):
    enc = fresh_a()
    ids, eos = _ids(3, 129, tc.VOCAB, 5), _eos(3, 129)
    base = _call(enc, ids, eos)                                              # synchronised: one handle serves one stream at a time
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        p, h = enc.encode_batch(ids, eos, want_hidden=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert _same((_bits(p), _bits(h)), base)


@pytest.mark.parametrize("B", (1, 3))
def test_out_pooled_of_exactly_B_rows_keeps_its_guards(fresh_a, L, dev, B):
    enc = fresh_a()
    T = 17
    ids, eos = _ids(B, T, tc.VOCAB, 6), _eos(B, T)
    want = _call(enc, ids, eos)[0]
    out = Out(dev, (B, enc.dim), F32)
    L.check(enc.lib.ch_text_encode(enc._h, ids.ctypes.data_as(I32P), eos.ctypes.data_as(I32P), B, T, out.ptr, None, L.stream_ptr()), "ch_text_encode")
    torch.cuda.synchronize()
    assert torch.equal(out.raw(), want)                                      # raw() checks both guard blocks first
