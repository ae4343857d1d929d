// Backward of the fused multi-head attention (head_dim 64, no mask; HF CLIPAttention as used by
// models/layers/adapter.py:127-177) for the ConceptHash training step -- one workgroup per (image, head), nothing but
// qkv and dO read, nothing but dqkv written; the probabilities are recomputed, never stored.
//
//   P = softmax(0.125 Q K^T),  O = P V                                   (forward, attention.hip)
//   dV = P^T dO,  dP = dO V^T,  D_q = sum_j P_qj dP_qj (= dO_q . O_q),  dS = 0.125 P o (dP - D),  dQ = dS K,  dK = dS^T Q
//
// LDS holds two [rows][128 B] images (attention_tile.h, filled by LDS-DMA): K and V during phase A, then --
// restaged between the phases -- Q and dO during phase B; the operands a phase needs only as per-lane fragments (Q / dO rows of
// the wave's query tile in A, K / V rows of its key tile in B) come straight from global memory, as the forward kernel reads Q.
// 59 KB instead of 118 KB, so TWO workgroups share a CU and cover each other's latencies (one was alone before).
// Phase A -- a wave owns 16-query tiles (the forward's layout: S^T = K Q^T, a lane holds one query's keys):
//   softmax statistics, dP^T = V dO^T, D_q, dS^T in registers; dQ^T = K^T dS^T with K^T from the hardware transpose read
//   (ds_read_b64_tr_b16), dS^T being already the B operand; (max, 1/sum, D_q) per query go to LDS.
// Phase B -- a wave owns 16-key tiles and walks the query tiles: bwd_key_tile_step (attention_tile.h) per (query tile, key tile).
//   The second S / dP product costs 4 MFMAs per tile pair and saves a round trip of P and dS through LDS.
#include "attention_tile.h"
#include "kernels.h"

namespace {

// EXT: an extra cotangent on the probabilities themselves -- dpext [B, heads, ncon, ntok - ncon - 1] fp32, the gradient of the
// concept-token attention rows the forward can tap (attention.hip TAP; consumer: the attention-diversity term of the loss,
// models/loss/coop.py:164-189) -- is added to dP = dO V^T on those (query, key) pairs, in both phases.
template <int KB, bool EXT>
__global__ __launch_bounds__(NW * 64, 4) void attention_bwd_kernel(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ dO, int ntok,
                                                               int heads, float scale_log2e, bf16_t *__restrict__ dqkv,
                                                               const float *__restrict__ dpext, int ncon) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KT = KB * 2;   // 16-row tiles
    constexpr int KP = KB * 32;  // padded rows (keys and queries)
    char *Ks = smem, *Vs = smem + KP * 128;    // phase A: K, V
    char *Qs = smem, *Gs = smem + KP * 128;    // phase B: Q, dO (same storage, restaged after phase A)
    f32x4 *stat = (f32x4 *)(smem + 2 * KP * 128);   // [KP]: lse (log2 domain), D_q / 8, -, -

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int D = heads * HD;
    const size_t ld = (size_t)3 * D;
    const bf16_t *base = qkv + (size_t)b * ntok * ld + h * HD;
    const bf16_t *gbase = dO + (size_t)b * ntok * D + h * HD;
    bf16_t *obase = dqkv + (size_t)b * ntok * ld + h * HD;

    stage_rows(base, ld, D, base, ld, 2 * D, 0, KP, ntok, Ks, Vs, wid, lane);

    const int fr = lane & 15, fq = lane >> 4;
    const int QT = (ntok + 15) >> 4;  // tiles holding at least one valid row
    const int npatch = ntok - ncon - 1, q_con0 = ntok - ncon;   // EXT: keys 1 .. npatch, queries q_con0 .. ntok - 1
    const ExtGrad ext{EXT ? dpext + (size_t)blockIdx.x * ncon * npatch : nullptr, npatch, q_con0};
    // frag_off / tr_off of attention_tile.h, written out, and the two fragment loads as a lambda: built from the header's Lane
    // (or its functions) and row_frag, the KB = 7 .. 9 instances spill 8 to 16 bytes per lane deeper
    // (profiles/attention_tile_registers.txt).  Same values: the header's rule is c ^ (row & 7), and (row & 7) of row 4*fq + tq is trow7.
    // b128 fragment of row (tile*16 + fr): d = 8*fq .. +8 (off0) and 32 + 8*fq .. (off1)
    const int off0 = fr * 128 + ((fq ^ (fr & 7)) << 4), off1 = fr * 128 + (((4 + fq) ^ (fr & 7)) << 4);
    // transpose read: lane 4*tq + tp of group fq addresses row 4*fq + tq of a 16-row tile, features 4*tp.. of feature tile dt
    const int tq = fr >> 2, tp = fr & 3;
    const int trow7 = ((fq & 1) << 2) | tq;
    int toff[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) toff[dt] = (fq * 4 + tq) * 128 + (((dt * 2 + (tp >> 1)) ^ trow7) << 4) + (tp & 1) * 8;

    // fragments of one 16-row tile straight from global memory: lane (row fr, fq) holds columns 8*fq.. and 32 + 8*fq.. of its row
    // (rows past the sequence re-read the last row: finite, masked / zero weight)
    auto row_frag = [&](const bf16_t *mat, size_t ldm, int tile, bf16x8 &f0, bf16x8 &f1) {
        const int r = min(tile * 16 + fr, ntok - 1);
        f0 = *(const bf16x8 *)(mat + (size_t)r * ldm + fq * 8);
        f1 = *(const bf16x8 *)(mat + (size_t)r * ldm + fq * 8 + 32);
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ================================ phase A: per query tile -> statistics and dQ ==========================================
    for (int qt = wid; qt < QT; qt += NW) {
        const int q = qt * 16 + fr;
        const bool qvalid = q < ntok;
        bf16x8 qf0, qf1, gf0, gf1;      // not prefetched a tile ahead: 16 VGPRs that the four-waves-per-SIMD budget does not have
        row_frag(base, ld, qt, qf0, qf1);
        row_frag(gbase, D, qt, gf0, gf1);
        // Register budget: only S^T / P^T of the tile (KT x 4 values) stays live; dP^T = V dO^T is RECOMPUTED where it is needed (once
        // for D_q, once for dS) instead of kept -- 28 more MFMAs per query tile on a pipe that is a quarter busy, 56 fewer VGPRs, so
        // that four waves per SIMD fit (the kernel is bound by its dependent LDS -> MFMA -> exp -> MFMA chains, not by throughput).
        f32x4 st[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) st[kt] = tile_mma(Ks, kt, off0, off1, Frag2{qf0, qf1});   // S^T[key = kt*16 + 4*fq + r][query fr]
        const bool ext_row = EXT && qt * 16 + 15 >= q_con0 && q >= q_con0 && qvalid;
        const float *erow = ext_row ? ext.ext + (size_t)(q - q_con0) * npatch : nullptr;
        auto dp_tile = [&](int kt) {   // dP^T[key = kt*16 + 4*fq + r][query fr] (+ the cotangent on the probabilities, EXT)
            f32x4 c = tile_mma(Vs, kt, off0, off1, Frag2{gf0, gf1});
            if constexpr (EXT) {
                if (ext_row) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = kt * 16 + fq * 4 + r;
                        if (key >= 1 && key <= npatch) c[r] += erow[key - 1];
                    }
                }
            }
            return c;
        };
        // keys >= ntok exist only in the last (KP - ntok + 15) / 16 <= 2 key tiles: mask those under a wave-uniform test (the PMC
        // counters show this kernel bound by VALU issue -- ~2,300 non-MFMA VALU instructions per wave against ~440 MFMAs)
#pragma unroll
        for (int kt = KT - 2; kt < KT; ++kt)
            if (kt >= 0 && kt * 16 + 16 > ntok) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + fq * 4 + r >= ntok) st[kt][r] = -1e30f;
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
        // (written out: through quad_sum, the spills of the EXT instances KB = 6 and 9 deepen by 4 and 8 bytes per lane)
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        float pd = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const f32x4 c = dp_tile(kt);
#pragma unroll
            for (int r = 0; r < 4; ++r) pd += st[kt][r] * c[r];
        }
        pd = quad_sum(pd);
        const float inv = 1.0f / sum;
        const float Dq = pd * inv;
        // per query for phase B: lse = mxs + log2(sum) so that P = exp2(s * scale_log2e - lse) needs no multiply by 1/sum (an invalid
        // query gets lse = 1e30 -> P = 0), and D_q / 8 so that dS = P * fma(dP, 0.125, -D_q/8): two VALU ops fewer per probability
        if (fq == 0) stat[q] = f32x4{qvalid ? mxs + __builtin_amdgcn_logf(sum) : 1e30f, 0.125f * Dq, 0.f, 0.f};
        // dS^T = 0.125 * P^T o (dP^T - D_q), as the bf16 B operand; logical k = 8*fq + j <-> key 32*kb + (j < 4 ? 4*fq + j : 16 + 4*fq + j - 4)
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float w = 0.125f * inv;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            PF pf;
            const f32x4 c0 = dp_tile(2 * kb), c1 = dp_tile(2 * kb + 1);
            pf.u[0] = pack_bf16x2(w * st[2 * kb][0] * (c0[0] - Dq), w * st[2 * kb][1] * (c0[1] - Dq));
            pf.u[1] = pack_bf16x2(w * st[2 * kb][2] * (c0[2] - Dq), w * st[2 * kb][3] * (c0[3] - Dq));
            pf.u[2] = pack_bf16x2(w * st[2 * kb + 1][0] * (c1[0] - Dq), w * st[2 * kb + 1][1] * (c1[1] - Dq));
            pf.u[3] = pack_bf16x2(w * st[2 * kb + 1][2] * (c1[2] - Dq), w * st[2 * kb + 1][3] * (c1[3] - Dq));
            VF kf[4];
            tr_unit(Ks, kb, toff, kf);
            unit_mma(o, kf, pf);
        }
        if (qvalid) store_o(obase + (size_t)q * ld + fq * 4, o);   // dQ[q][dt*16 + 4*fq + r]
    }
    __syncthreads();   // every wave is done with K and V in LDS, the statistics are complete
    stage_rows(base, ld, 0, gbase, D, 0, 0, KP, ntok, Qs, Gs, wid, lane);   // restage: Q and dO take the place of K and V
    bf16x8 k0, k1, v0, v1;   // this wave's first key tile, from global, under the restaging
    if (wid < QT) {
        row_frag(base + D, ld, wid, k0, k1);
        row_frag(base + 2 * D, ld, wid, v0, v1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ================================ phase B: per key tile -> dK, dV ========================================================
    for (int kt = wid; kt < QT; kt += NW) {
        const int key = kt * 16 + fr;
        const bool kvalid = key < ntok;
        const bool edge_tile = kt * 16 + 16 > ntok;
        if (kt != wid) {
            row_frag(base + D, ld, kt, k0, k1);
            row_frag(base + 2 * D, ld, kt, v0, v1);
        }
        f32x4 dkt[4], dvt[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dkt[dt] = dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qt = 0; qt < QT; ++qt)
            bwd_key_tile_step<EXT>(Qs, Gs, qt, qt, Frag2{k0, k1}, Frag2{v0, v1}, stat, scale_log2e, key, edge_tile && !kvalid, ntok, ext, off0, off1,
                                   toff, fq, dkt, dvt);
        if (kvalid) {
            bf16_t *kp = obase + (size_t)key * ld + D + fq * 4;
            store_o(kp, dkt);
            store_o(kp + D, dvt);
        }
    }
}

template <int KB, bool EXT>
int launch_bwd_inst(const bf16_t *qkv, const bf16_t *dO, int B, int ntok, int heads, bf16_t *dqkv, const float *dpext, int ncon, hipStream_t s) {
    constexpr int KP = KB * 32;
    const size_t lds = (size_t)KP * 128 * 2 + (size_t)KP * 16;
    CH_REQUIRE(lds <= 160 * 1024, "attention backward: sequence too long for the LDS-resident kernel");
    static ch_once_per_device lds_once;
    if (int e = ch_func_max_lds((const void *)attention_bwd_kernel<KB, EXT>, (int)lds, lds_once)) return e;
    hipLaunchKernelGGL((attention_bwd_kernel<KB, EXT>), dim3(B * heads), dim3(NW * 64), lds, s, qkv, dO, ntok, heads, ATTN_SCALE_LOG2E, dqkv,
                       dpext, ncon);
    CH_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// qkv [B*ntok, 3D] bf16 (q | k | v), dO [B*ntok, D] bf16 -> dqkv [B*ntok, 3D] bf16 (dq | dk | dv); head_dim 64
// dpext (optional): [B, heads, ncon, ntok - ncon - 1] fp32 cotangent of the concept tokens' attention rows over the patch tokens
int ch_attention_bwd(const bf16_t *qkv, const bf16_t *dO, int B, int ntok, int heads, bf16_t *dqkv, hipStream_t s, const float *dpext,
                     int ncon, int kernel) {
    CH_REQUIRE(B > 0 && ntok > 0 && heads > 0, "attention backward: empty problem");
    CH_REQUIRE(!dpext || (ncon >= 1 && ncon < ntok - 1), "attention backward: the probability cotangent needs 1 <= ncon < ntok - 1");
    CH_REQUIRE(kernel >= 0 && kernel <= 2, "attention backward: kernel must be 0 (by length), 1 (resident) or 2 (streaming)");
    if (kernel == 2 || (kernel == 0 && ntok > CH_ATTN_RESIDENT_MAX_TOKENS)) {   // attention_stream.hip
        ch_attention_count_launch(3);
        return ch_attention_bwd_stream(qkv, dO, B, ntok, heads, dqkv, s, dpext, ncon);
    }
    if (ntok <= CH_ATTN_RESIDENT_MAX_TOKENS) ch_attention_count_launch(2);
    const int rc = ch_attn_dispatch_kb((ntok + 31) / 32, [&](auto kb) {
        return dpext ? launch_bwd_inst<decltype(kb)::value, true>(qkv, dO, B, ntok, heads, dqkv, dpext, ncon, s)
                     : launch_bwd_inst<decltype(kb)::value, false>(qkv, dO, B, ntok, heads, dqkv, nullptr, 0, s);
    });
    if (rc >= 0) return rc;
    ch_set_error("attention backward: the LDS-resident kernel holds at most 288 tokens per image");
    return 2;
}
