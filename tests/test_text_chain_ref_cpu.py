"""CPU: the references of tests/text_chain_ref.py are (a) sound -- an fp32 emulation in ANOTHER summation order stays inside the new bound
of text_pool_kernel on every row family, width, row count and eps of tests/test_text_chain_gpu.py, and equals the bit-exact reference of
text_embed_kernel -- and (b) sharp -- every listed defect leaves the bound (or the bit-exact comparison) on at least one of those inputs,
and every case catches at least one.  `compose`, chained in fp64 without intermediate rounding, is the fp32 restatement
tests/text_tower_ref.text_forward (itself pinned against transformers) up to that restatement's own fp32 noise, for both activations: the
q | k | v stacking, the stage order and the residual wiring are the Hugging Face ones.  The worst clean ratio is printed (-s).  No GPU,
no library."""
import torch

import text_chain_ref as tc
import text_tower_ref as ttr
import train_kernels_ref as tr
from test_train_kernels_ref_cpu import Tally


def test_embed_is_exact_and_every_index_defect_shows():
    caught = set()
    for D in tc.EMBED_D:
        for B, T in tc.EMBED_BT:
            ids, tok, pos = tc.embed_inputs(B, T, D)
            assert int(ids.max()) == tc.VOCAB - 1 and (B * T == 1 or int(ids.min()) == 0)
            want = tc.embed_ref(ids, T, tok, pos)
            assert want.shape == (B * T, D) and tr.bits_equal(tc.embed_emul(ids, T, tok, pos), want), (D, B, T)
            hits = {d for d in tc.EMBED_DEFECTS if not tr.bits_equal(tc.embed_emul(ids, T, tok, pos, d), want)}
            # the position defect needs a second prompt, the token defect a second row
            assert ("pos_of_row" in hits) == (B > 1) and ("tok_of_neighbour" in hits) == (B * T > 1), (D, B, T, hits)
            caught |= hits
    assert caught == set(tc.EMBED_DEFECTS)


def test_pool_every_row_family_and_defect():
    t = Tally("text_pool", tc.POOL_DEFECTS)
    for D in tc.POOL_D:
        w, b = tc.fr.affine_params(D, "final")
        for eps in tc.POOL_EPS:
            for fam in tc.ROW_FAMILIES:
                for rows in tc.POOL_ROWS:                                    # every row
                    H = tc.row_family(fam, rows, D, "pool")
                    ref, bound = tc.pool_ref(H, None, 1, w, b, eps)
                    what = f"{fam} {rows}x{D} eps {eps}"
                    t.clean(tc.pool_emul(H, None, 1, w, b, eps), ref, bound, what)
                    hits = {d: tr.breaches(tc.pool_emul(H, None, 1, w, b, eps, d), ref, bound) for d in tc.POOL_DEFECTS}
                    assert hits["pool_through_bf16"], what                   # an fp32 output: four orders of magnitude below a bf16 ulp
                    assert not hits["eos_plus_1"] and not hits["eos_stride_max_positions"]      # no eos in this mode
                    if fam == "offset" and rows == 37:
                        assert hits["one_pass"], what
                    t.case(what, hits)
                for B, T, eos in tc.POOL_EOS:                                # the eos gather
                    H = tc.row_family(fam, B * T, D, "pool_eos")
                    e = torch.tensor(eos, dtype=torch.int32)
                    ref, bound = tc.pool_ref(H, e, T, w, b, eps)
                    what = f"{fam} eos {B}x{T} D {D} eps {eps}"
                    assert ref.shape == (B, D)
                    # eos mode reads rows of the all-rows result: the same reference rows
                    full, _ = tc.pool_ref(H, None, T, w, b, eps)
                    assert torch.equal(ref, full[torch.arange(B) * T + e.long()])
                    t.clean(tc.pool_emul(H, e, T, w, b, eps), ref, bound, what)
                    hits = {d: tr.breaches(tc.pool_emul(H, e, T, w, b, eps, d), ref, bound) for d in tc.POOL_DEFECTS}
                    if B > 1:
                        assert hits["eos_plus_1"] and hits["eos_stride_max_positions"], what
                    t.case(what, hits)
    t.done()


def test_the_pool_bound_is_the_row_kernels_bound_without_the_bf16_term():
    """same n, same two-pass terms as layernorm_ref on the same rows: the same reference, and the bf16 output's bound is this one plus
    the half ulp of the rounded value"""
    for D in tc.POOL_D:
        for fam in tc.ROW_FAMILIES:
            H = tc.row_family(fam, 37, D, "pool")
            w, b = tc.fr.affine_params(D, "final")
            ref, bound = tc.pool_ref(H, None, 1, w, b, 1e-5)
            ref2, bound2 = tc.fr.layernorm_ref(H, w, b, tc.fr.n_row_stats(D))
            assert torch.equal(ref, ref2) and bool(torch.isfinite(bound).all())
            assert torch.equal(bound2, tr.bf16_out(ref, bound))


def test_compose_is_the_hugging_face_layer():
    """compose chained in fp64 against the fp32 restatement on the same (bf16-rounded) weights.  The restatement is fp32 throughout: its
    own noise on these two-layer towers is a few gam(K) of an O(1) activation, K <= 384, i.e. ~1e-5 of the output's RMS (DESIGN.md records
    2e-5 between it and transformers); a wiring slip -- k for q, a stage out of order, the wrong activation, a residual taken before the
    LayerNorm -- moves the output by more than 1e-2 of it.  1e-4 separates the two by two orders of magnitude on either side."""
    for dims, heads, act, eps, B, T in ((dict(hidden_size=128, intermediate_size=256), 2, "quick_gelu", 1e-5, 3, 17),
                                        (dict(hidden_size=128, intermediate_size=256), 2, "gelu", 1e-6, 2, 33),
                                        (dict(hidden_size=384, intermediate_size=384), 6, "quick_gelu", 1e-5, 2, 9)):
        dims = dict(dims, vocab_size=tc.VOCAB, max_position_embeddings=40, num_hidden_layers=2, num_attention_heads=heads)
        sd = ttr.seeded_text_state_dict(dims, seed=3)
        for k in list(sd):                                  # the weights both sides use: what the loader keeps
            if k.endswith("proj.weight") or k.endswith("fc1.weight") or k.endswith("fc2.weight"):
                sd[k] = sd[k].to(torch.bfloat16).float()
        ids = torch.randint(0, tc.VOCAB, (B, T), generator=tc.gen("compose", B, T))
        want, _ = ttr.text_forward(sd, ids, heads=heads, act=act, eps=eps)
        got = tc.compose_forward(sd, ids, heads, 2, act, eps)
        rms = float(want.double().pow(2).mean().sqrt())
        err = float((got - want.double()).abs().max()) / rms
        print(f"compose vs text_forward, D {dims['hidden_size']} {act}: max-abs / RMS {err:.2e}")
        assert err < 1e-4, err
        # and the wrong activation, or q and k exchanged, is far outside
        other = tc.compose_forward(sd, ids, heads, 2, "gelu" if act == "quick_gelu" else "quick_gelu", eps)
        assert float((other - want.double()).abs().max()) / rms > 1e-2
        swapped = {k.replace("q_proj", "X").replace("k_proj", "q_proj").replace("X", "k_proj"): v for k, v in sd.items()}
        if T > 1:
            assert float((tc.compose_forward(swapped, ids, heads, 2, act, eps) - want.double()).abs().max()) / rms > 1e-2
