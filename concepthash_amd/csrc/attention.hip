// Multi-head self-attention for the ConceptHash ViT encoder (gfx950): head_dim 64, sequence 54..288 tokens, no mask.
// (Longer sequences: attention_stream.hip; ch_attention below chooses by length.)
//
// Restates HF CLIPAttention's eager path (transformers modeling_clip.py eager_attention_forward: softmax(q k^T / sqrt(d)) v)
// as called from the reference's CLIPEncoderLayerWithAdapter.forward (models/layers/adapter.py:146-152).  The reference
// materialises every layer's (B,heads,N,N) probability map (output_attentions=True, models/arch/coop.py:474-479); retrieval
// never reads it, so this kernel keeps scores in registers and never writes them.
//
// One workgroup (8 waves) per (image, head).  The head's whole K and V are staged ROW-MAJOR into LDS by LDS-DMA (no VGPR
// round trip, all 14 requests of a wave in flight at once) as two swizzled images; the image rule, the lane geometry that reads
// it and the tile primitives are attention_tile.h's.  Each wave takes 16-query tiles round robin:
//   S^T = K Q^T      16x16x32 bf16 MFMAs with A = K tile (ds_read_b128, conflict free), B = Q^T fragment straight
//                    from global: a lane holds, for ONE query (lane & 15), 4 consecutive keys per 16-key tile, so the
//                    softmax reductions are in-register plus two cross-lane steps (xor 16, xor 32);
//   O^T = V^T P^T    the exponentiated scores, converted to bf16 in place, already ARE the B operand of this product; the
//                    A operand V^T comes from the row-major V image through the hardware transpose read
//                    ds_read_b64_tr_b16 (a 16-lane group fetches 4 keys x 16 features and each lane receives one feature
//                    column) -- conflict free with the same swizzle.  P never goes through LDS.
//   out = O / rowsum (fp32), 4 consecutive d per lane -> 8-byte bf16 stores.
#include "attention_tile.h"
#include "kernels.h"

namespace {

// KB: number of 32-key blocks (keys padded to KB*32); TAP: write the concept-token attention rows; COMPACT: only the rows the
// hashing head reads -- CLS and the `ncon` concept tokens -- are queries, and the output is [B * (1 + ncon), D] (final layer);
// CAUSAL: query q sees keys 0..q only (the CLIP text tower, text_model.hip; never with TAP or COMPACT)
template <int KB, bool TAP, bool COMPACT, bool CAUSAL = false>
__global__ __launch_bounds__(NW * 64, 4) void attention_kernel(const bf16_t *__restrict__ qkv, int ntok, int heads, float scale_log2e,
                                                        bf16_t *__restrict__ out, float *__restrict__ cattn, int ncon, int rev) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KT = KB * 2;   // 16-key tiles
    constexpr int KP = KB * 32;  // padded keys
    char *Ks = smem;             // [KP][128 B]
    char *Vs = smem + KP * 128;  // [KP][128 B]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = rev ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int b = bid / heads, h = bid - b * heads;
    const int D = heads * HD;
    const size_t ld = (size_t)3 * D;
    const bf16_t *base = qkv + (size_t)b * ntok * ld + h * HD;

    stage_rows(base, ld, D, base, ld, 2 * D, 0, KP, ntok, Ks, Vs, wid, lane);   // the head's whole K and V

    const int fr = lane & 15, fq = lane >> 4;
    const int nqc = 1 + ncon;  // COMPACT: queries per image
    const int QT = COMPACT ? (nqc + 15) >> 4 : (ntok + 15) >> 4;
    // first query tile's Q fragments overlap the staging latency
    bool qvalid;
    int qslot = wid * 16 + fr;
    int q = query_slot<COMPACT>(qslot, ntok, ncon, nqc, qvalid);
    Frag2 qf = ld_frag(base, ld, q, fq);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const Lane g(lane);   // after the barrier: built above it, KB = 4 (tap) and KB = 5 lose their fifth wave per SIMD

    for (int qt = wid; qt < QT; qt += NW) {
        // S^T in chunks of two key tiles, fragment reads of chunk c+1 issued before the MFMAs of chunk c; the scheduling fences
        // keep the compiler from hoisting all 28 reads (112 VGPRs) above the first MFMA, which costs the third wave per SIMD
        f32x4 st[KT];
        Frag2 kf[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) kf[0][t] = tile_frag(Ks, t, g.off0, g.off1);
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            if (c + 1 < KB) {
#pragma unroll
                for (int t = 0; t < 2; ++t) kf[(c + 1) & 1][t] = tile_frag(Ks, 2 * c + 2 + t, g.off0, g.off1);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) st[2 * c + t] = mma2(kf[c & 1][t], qf);
            __builtin_amdgcn_sched_barrier(0);
        }
        const bool cur_valid = qvalid;
        const int cur_q = q, cur_slot = qslot;
        // prefetch the next tile's Q fragments
        if (qt + NW < QT) {
            qslot = (qt + NW) * 16 + fr;
            q = query_slot<COMPACT>(qslot, ntok, ncon, nqc, qvalid);
            qf = ld_frag(base, ld, q, fq);
        }
        // ---- softmax over keys for query (lane & 15): lane holds keys kt*16 + 4*fq + r
        // keys >= ntok exist only in the last (KP - ntok + 15) / 16 <= 2 key tiles: mask those under a wave-uniform test
        // (mask_tail written out: through the helper the KB <= 4 instances change their occupancy step)
#pragma unroll
        for (int kt = KT - 2; kt < KT; ++kt)
            if (kt >= 0 && kt * 16 + 16 > ntok) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + fq * 4 + r >= ntok) st[kt][r] = -1e30f;
            }
        // causal: one select per score (query = lane & 15), straight-line so that register allocation stays the plain instance's;
        // key 0 is never masked, so every row keeps a finite maximum and the masked keys get probability exactly 0
        if constexpr (CAUSAL) {
            const int lim = cur_q - fq * 4;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) st[kt][r] = kt * 16 + r > lim ? -1e30f : st[kt][r];
        }
        float mx = -1e30f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[kt][r]);
        mx = quad_max(mx);
        const float mxs = mx * scale_log2e;
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(st[kt][r] * scale_log2e - mxs);
                st[kt][r] = e;
                sum += e;
            }
        sum = quad_sum(sum);
        const float inv = 1.0f / sum;
        // optional interpretability tap (last layer only): softmax rows of the `ncon` concept tokens over the patch tokens,
        // = attn_cache[-1][:, :, -Q:, 1:-Q] of the reference (models/arch/coop.py:481-482, models/loss/coop.py:164-176)
        if (TAP && cur_valid && cur_q >= ntok - ncon) {
            const int np = ntok - ncon - 1;
            float *dst = cattn + (((size_t)b * heads + h) * ncon + (cur_q - (ntok - ncon))) * np;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt * 16 + fq * 4 + r;
                    if (key >= 1 && key <= np) dst[key - 1] = st[kt][r] * inv;
                }
        }

        // ---- O^T = V^T P^T ; logical k = 8*fq + j  <->  key 32*kb + (j < 4 ? 4*fq + j : 16 + 4*fq + j - 4)
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        VF vf[2][4];
        // keys 32kb + 4fq + 0..3 (elements 0..3) and + 16 (elements 4..7): immediate offsets off one lane base
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            vf[0][dt].h[0] = tr_read(Vs + g.toff[dt]);
            vf[0][dt].h[1] = tr_read(Vs + TILE_BYTES + g.toff[dt]);
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            if (kb + 1 < KB) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    vf[(kb + 1) & 1][dt].h[0] = tr_read(Vs + (kb + 1) * UNIT_BYTES + g.toff[dt]);
                    vf[(kb + 1) & 1][dt].h[1] = tr_read(Vs + (kb + 1) * UNIT_BYTES + TILE_BYTES + g.toff[dt]);
                }
            }
            const PF pf = pack8(st[2 * kb], st[2 * kb + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = mma_acc(vf[kb & 1][dt], pf, o[dt]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (cur_valid) store_o(out + (COMPACT ? (size_t)b * nqc + cur_slot : (size_t)b * ntok + cur_q) * D + h * HD + fq * 4, o, inv);
    }
}

template <int KB, bool TAP, bool COMPACT, bool CAUSAL = false>
int launch_attn_inst(const bf16_t *qkv, int B, int ntok, int heads, bf16_t *out, float *cattn, int ncon, int rev, hipStream_t s) {
    const int KP = KB * 32;
    const size_t lds = (size_t)KP * 128 * 2;
    CH_REQUIRE(lds <= 160 * 1024, "attention: sequence too long for the LDS-resident K/V kernel");
    static ch_once_per_device lds_once;
    if (int e = ch_func_max_lds((const void *)attention_kernel<KB, TAP, COMPACT, CAUSAL>, (int)lds, lds_once)) return e;
    CH_LAUNCH((attention_kernel<KB, TAP, COMPACT, CAUSAL>), dim3(B * heads), dim3(NW * 64), lds, s, qkv, ntok, heads, ATTN_SCALE_LOG2E,
                       out, cattn, ncon, rev);
    CH_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int ch_attention(const bf16_t *qkv, int B, int ntok, int heads, bf16_t *out, hipStream_t s, float *cattn, int ncon, bool compact,
                 bool rev, int kernel) {
    CH_REQUIRE(B > 0 && ntok > 0 && heads > 0, "attention: empty problem");
    CH_REQUIRE(!compact || (ncon >= 1 && ncon < ntok), "attention: compact mode needs 1 <= ncon < ntok");
    CH_REQUIRE(kernel >= 0 && kernel <= 2, "attention: kernel must be 0 (by length), 1 (resident) or 2 (streaming)");
    if (kernel == 2 || (kernel == 0 && ntok > CH_ATTN_RESIDENT_MAX_TOKENS)) {   // attention_stream.hip
        ch_attention_count_launch(1);
        return ch_attention_stream(qkv, B, ntok, heads, out, s, cattn, ncon, compact, rev);
    }
    if (ntok <= CH_ATTN_RESIDENT_MAX_TOKENS) ch_attention_count_launch(0);
    const int r = rev ? 1 : 0;
    const int rc = ch_attn_dispatch_kb((ntok + 31) / 32, [&](auto kb) {
        return ch_attn_pick_mode(cattn != nullptr, compact, [&](auto tap, auto cmp) {
            return launch_attn_inst<decltype(kb)::value, decltype(tap)::value, decltype(cmp)::value>(qkv, B, ntok, heads, out, cattn, ncon, r, s);
        });
    });
    if (rc >= 0) return rc;
    ch_set_error("attention: the LDS-resident kernel holds at most 288 tokens per image");
    return 2;
}

// Causal self-attention of the CLIP text tower (text_model.hip): the resident kernel's CAUSAL instance, no tap, no compact mode.
int ch_attention_causal(const bf16_t *qkv, int B, int ntok, int heads, bf16_t *out, hipStream_t s) {
    CH_REQUIRE(B > 0 && ntok > 0 && heads > 0, "causal attention: empty problem");
    CH_REQUIRE(ntok <= CH_ATTN_RESIDENT_MAX_TOKENS, "causal attention: the LDS-resident kernel holds at most 288 tokens per sequence");
    return ch_attn_dispatch_kb((ntok + 31) / 32, [&](auto kb) {   // 1 <= KB <= 9 by the two checks above
        return launch_attn_inst<decltype(kb)::value, false, false, true>(qkv, B, ntok, heads, out, nullptr, 0, 0, s);
    });
}
