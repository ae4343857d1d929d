// Streaming multi-head self-attention, forward and backward, for sequences past the 288 tokens that the LDS-resident kernels
// (attention.hip, attention_bwd.hip) hold: head_dim 64, no mask, up to CH_ATTN_MAX_TOKENS tokens (a 32 x 32 patch grid).
//
// Same arithmetic (HF CLIPAttention eager path, softmax(q k^T / sqrt(d)) v) and the same tile vocabulary as the resident kernels
// (attention_tile.h: LDS image, lane geometry, staging, tile primitives) -- only the walk differs: the sequence is taken in blocks
// of BK = 64 rows that are staged into a two-deep LDS ring: the block after the one being computed is in flight (LDS-DMA) while the
// MFMAs run, and one barrier per block both publishes the landed block and frees the buffer the next one goes into.  41 KB of LDS
// at 1,029 tokens for the backward, 32 KB for the forward, at any length.
//
// Forward: one workgroup per (image, head, chunk of 128 queries); a wave owns one 16-query tile and keeps, per query, a running
//   maximum and a running sum in fp32 (online softmax): per block  m' = max(m, max_j s_j),  alpha = exp2((m - m') c),
//   l = alpha l + sum_j p_j,  O = alpha O + P V  with  p_j = exp2((s_j - m') c)  rounded to bf16 as the B operand of the P V
//   product, exactly where the resident kernel rounds it; out = O / l.  The TAP rows (the concept tokens' probabilities over the
//   patch tokens) need the FINAL (m, l): the waves whose tile holds concept tokens make a second pass over the keys -- K fragments
//   straight from global memory, two MFMAs per 16 keys, no V -- and write  exp2((s - m) c) / l.  At most five of a (image, head)'s
//   query tiles do (ncontext <= 64), one with the shipped four concept tokens.
// Backward: one workgroup per (image, head), nothing but qkv and dO read, nothing but dqkv written, no atomics: every output
//   element is accumulated by ONE wave in registers in a fixed order, so a launch is run-to-run bit-identical.
//   Phase A, per chunk of 128 queries (a wave owns a 16-query tile), TWO walks over the key blocks (K and V staged):
//     walk 1: running (m, l) and the running  sum_j p_j (dP_j + ext_j)  ->  lse = m c + log2 l,  D_q = sum / l   (recomputed, not
//             read from the saved forward output: the last layer's saved output holds only the head rows, and the cotangent on the
//             probabilities (EXT) adds sum_j P_qj ext_qj to D_q, which dO . O does not contain) -> LDS, 8 bytes per query;
//     walk 2: P = exp2(s c - lse), dS = 0.125 P (dP - D_q) as the bf16 B operand, dQ^T += K^T dS^T.
//   Phase B, per chunk of 128 keys (a wave owns a 16-key tile, its K / V fragments from global memory), one walk over the query
//     blocks (Q and dO staged): S and dP in the transposed lane layout, P and dS rebuilt from the statistics in LDS,
//     dV^T += dO^T P, dK^T += Q^T dS by the 16x16x16 bf16 MFMA -- the resident kernel's phase B, block by block.
#include "attention_tile.h"
#include "kernels.h"

namespace {

constexpr int BK = 64;                       // rows (keys, or queries in the backward's phase B) per staged block: one LDS-DMA pair per wave
constexpr int BT = BK / 16;                  // 16-row tiles per block
constexpr int BU = BK / 32;                  // 32-key units (one PV MFMA's reduction depth) per block
constexpr int STAGE_BYTES = 2 * BK * 128;    // two matrices per stage

// rows [r0, r0 + BK) of two column blocks -> buf (first) and buf + BK * 128 (second)
__device__ __forceinline__ void stage_block(const bf16_t *a, size_t lda, const bf16_t *b, size_t ldb, int r0, int ntok, char *buf, int wid,
                                            int lane) {
    stage_rows(a, lda, 0, b, ldb, 0, r0, BK, ntok, buf, buf + BK * 128, wid, lane);
}

// TAP: write the concept-token attention rows; COMPACT: only CLS and the `ncon` concept tokens are queries, out is [B * (1 + ncon), D]
template <bool TAP, bool COMPACT>
__global__ __launch_bounds__(NW * 64, 4) void attention_stream_kernel(const bf16_t *__restrict__ qkv, int ntok, int heads, float scale_log2e,
                                                                   bf16_t *__restrict__ out, float *__restrict__ cattn, int ncon, int rev) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // two stages of [K block | V block]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = rev ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const int b = bid / heads, h = bid - b * heads;
    const int D = heads * HD;
    const size_t ld = (size_t)3 * D;
    const bf16_t *base = qkv + (size_t)b * ntok * ld + h * HD;
    const int NB = (ntok + BK - 1) / BK;

    stage_block(base + D, ld, base + 2 * D, ld, 0, ntok, smem, wid, lane);

    const int fr = lane & 15, fq = lane >> 4;
    const int nqc = 1 + ncon;  // COMPACT: queries per image
    const int QT = COMPACT ? (nqc + 15) >> 4 : (ntok + 15) >> 4;
    const int qt = (int)blockIdx.y * NW + wid;
    const bool active = qt < QT;   // wave-uniform; an idle wave of the last chunk still stages its share and meets every barrier
    // query slot j of this image -> (token row, valid), as attention.hip
    const int qslot = qt * 16 + fr;
    bool qvalid;
    const int q = query_slot<COMPACT>(qslot, ntok, ncon, nqc, qvalid);
    const Frag2 qf = ld_frag(base, ld, q, fq);
    const Lane g(lane);

    float m = -1e30f, l = 0.f;   // running maximum (raw score units) and this lane's share of the running sum
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j = 0; j < NB; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of block j has landed
        __syncthreads();                                   // ... everyone's has, and everyone is done with block j - 1
        if (j + 1 < NB) stage_block(base + D, ld, base + 2 * D, ld, (j + 1) * BK, ntok, smem + ((j + 1) & 1) * STAGE_BYTES, wid, lane);
        if (!active) continue;
        const char *Ks = smem + (j & 1) * STAGE_BYTES, *Vs = Ks + BK * 128;
        f32x4 st[BT];   // S^T[key = j*BK + t*16 + 4*fq + r][query fr]
#pragma unroll
        for (int t = 0; t < BT; ++t) st[t] = tile_mma(Ks, t, g.off0, g.off1, qf);
        if (j * BK + BK > ntok) {   // only the last block has keys past the sequence (wave-uniform test)
#pragma unroll
            for (int t = 0; t < BT; ++t) st[t] = mask_tail(st[t], j * BK + t * 16, ntok, fq);
        }
        float bm = -1e30f;
#pragma unroll
        for (int t = 0; t < BT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) bm = fmaxf(bm, st[t][r]);
        bm = quad_max(bm);
        const float mn = fmaxf(m, bm);   // every block holds at least one real key: finite from the first block on
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);   // first block: exp2(-huge) = 0 on O = 0, l = 0
        const float mns = mn * scale_log2e;
        m = mn;
        float bs = 0.f;
#pragma unroll
        for (int t = 0; t < BT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(st[t][r] * scale_log2e - mns);
                st[t][r] = e;
                bs += e;
            }
        l = l * alpha + bs;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
        // O^T += V^T P^T ; logical k = 8*fq + i  <->  key 32*u + (i < 4 ? 4*fq + i : 16 + 4*fq + i - 4)
#pragma unroll
        for (int u = 0; u < BU; ++u) {
            VF vf[4];
            tr_unit(Vs, u, g.toff, vf);
            unit_mma(o, vf, pack8(st[2 * u], st[2 * u + 1]));
        }
    }
    if (!active) return;   // no barrier below
    l = quad_sum(l);
    const float inv = 1.0f / l;
    if constexpr (TAP) {
        // second pass for the tiles that hold concept tokens: their rows over the patch tokens with the final statistics
        // (= attn_cache[-1][:, :, -Q:, 1:-Q] of the reference, models/arch/coop.py:481-482)
        const bool crow = qvalid && q >= ntok - ncon;
        if (__builtin_amdgcn_ballot_w64(crow) != 0) {
            const int np = ntok - ncon - 1;
            float *dst = cattn + (((size_t)b * heads + h) * ncon + (crow ? q - (ntok - ncon) : 0)) * np;
            const float ms = m * scale_log2e;
            const int KT = (ntok + 15) >> 4;
            for (int kt = 0; kt < KT; ++kt) {
                const f32x4 a = mma2(row_frag(base + D, ld, kt * 16 + fr, ntok, fq), qf);
                if (crow) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = kt * 16 + fq * 4 + r;
                        if (key >= 1 && key <= np) dst[key - 1] = __builtin_amdgcn_exp2f(a[r] * scale_log2e - ms) * inv;
                    }
                }
            }
        }
    }
    if (qvalid) store_o(out + (COMPACT ? (size_t)b * nqc + qslot : (size_t)b * ntok + q) * D + h * HD + fq * 4, o, inv);
}

// EXT: dpext [B, heads, ncon, ntok - ncon - 1] fp32, the cotangent of the tapped probability rows, is added to dP on those
// (query, key) pairs in both phases (attention_bwd.hip)
template <bool EXT>
__global__ __launch_bounds__(NW * 64, 4) void attention_bwd_stream_kernel(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ dO, int ntok,
                                                                       int heads, float scale_log2e, bf16_t *__restrict__ dqkv,
                                                                       const float *__restrict__ dpext, int ncon) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x2 *stat = (f32x2 *)(smem + 2 * STAGE_BYTES);   // [NB * BK]: lse (log2 domain), D_q / 8

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int D = heads * HD;
    const size_t ld = (size_t)3 * D;
    const bf16_t *base = qkv + (size_t)b * ntok * ld + h * HD;
    const bf16_t *gbase = dO + (size_t)b * ntok * D + h * HD;
    bf16_t *obase = dqkv + (size_t)b * ntok * ld + h * HD;
    const int NB = (ntok + BK - 1) / BK;
    const int QT = (ntok + 15) >> 4;        // 16-row tiles holding at least one valid row
    const int NC = (QT + NW - 1) / NW;      // chunks of NW tiles (queries in phase A, keys in phase B)

    stage_block(base + D, ld, base + 2 * D, ld, 0, ntok, smem, wid, lane);
    // rows past the sequence: lse = 1e30 -> P = 0 in phase B (phase A writes the valid rows only)
    for (int i = ntok + tid; i < NB * BK; i += NW * 64) stat[i] = f32x2{1e30f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    const int npatch = ntok - ncon - 1, q_con0 = ntok - ncon;   // EXT: keys 1 .. npatch, queries q_con0 .. ntok - 1
    const float *ext = EXT ? dpext + (size_t)blockIdx.x * ncon * npatch : nullptr;
    const Lane g(lane);
    const int off0 = g.off0, off1 = g.off1;
    const int (&toff)[4] = g.toff;
    // fragments of one 16-row tile straight from global memory (rows past the sequence re-read the last row)
    auto row_frag = [&](const bf16_t *mat, size_t ldm, int tile, bf16x8 &f0, bf16x8 &f1) {
        const int r = min(tile * 16 + fr, ntok - 1);
        f0 = *(const bf16x8 *)(mat + (size_t)r * ldm + fq * 8);
        f1 = *(const bf16x8 *)(mat + (size_t)r * ldm + fq * 8 + 32);
    };

    // ================================ phase A: per query tile -> statistics (walk 1), dQ (walk 2) ============================
    {
        bf16x8 qf0 = {}, qf1 = {}, gf0 = {}, gf1 = {};
        float m = -1e30f, l = 0.f, pd = 0.f, lse = 0.f, Dq = 0.f;
        int q = 0;
        bool qvalid = false, ext_row = false;
        const float *erow = nullptr;
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int total = NC * 2 * NB;
        int qc = 0, rem = 0;   // step = qc * 2 NB + rem
        for (int step = 0; step < total; ++step) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (step + 1 < total) {
                int nb = rem + 1;
                nb = nb >= 2 * NB ? 0 : (nb >= NB ? nb - NB : nb);
                stage_block(base + D, ld, base + 2 * D, ld, nb * BK, ntok, smem + ((step + 1) & 1) * STAGE_BYTES, wid, lane);
            }
            const int walk = rem >= NB ? 1 : 0, j = rem - walk * NB;
            const int qt = qc * NW + wid;
            const int cur_rem = rem;
            if (++rem == 2 * NB) {
                rem = 0;
                ++qc;
            }
            if (qt >= QT) continue;   // wave-uniform
            if (cur_rem == 0) {
                q = qt * 16 + fr;
                qvalid = q < ntok;
                row_frag(base, ld, qt, qf0, qf1);
                row_frag(gbase, D, qt, gf0, gf1);
                m = -1e30f;
                l = 0.f;
                pd = 0.f;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
                ext_row = EXT && q >= q_con0 && qvalid;
                erow = ext_row ? ext + (size_t)(q - q_con0) * npatch : nullptr;
            }
            const char *Ks = smem + (step & 1) * STAGE_BYTES, *Vs = Ks + BK * 128;
            f32x4 st[BT], dp[BT];   // S^T and dP^T [key = j*BK + t*16 + 4*fq + r][query fr]
#pragma unroll
            for (int t = 0; t < BT; ++t) {
                const Frag2 kt2 = tile_frag(Ks, t, off0, off1), vt2 = tile_frag(Vs, t, off0, off1);
                const f32x4 a = mma2(kt2, Frag2{qf0, qf1});
                f32x4 c = mma2(vt2, Frag2{gf0, gf1});
                if constexpr (EXT) {
                    if (ext_row) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int key = j * BK + t * 16 + fq * 4 + r;
                            if (key >= 1 && key <= npatch) c[r] += erow[key - 1];
                        }
                    }
                }
                st[t] = a;
                dp[t] = c;
            }
            if (j * BK + BK > ntok) {   // only the last block has keys past the sequence (wave-uniform test)
#pragma unroll
                for (int t = 0; t < BT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (j * BK + t * 16 + fq * 4 + r >= ntok) st[t][r] = -1e30f;
            }
            if (walk == 0) {
                float bm = -1e30f;
#pragma unroll
                for (int t = 0; t < BT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) bm = fmaxf(bm, st[t][r]);
                bm = quad_max(bm);
                const float mn = fmaxf(m, bm);
                const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);
                const float mns = mn * scale_log2e;
                m = mn;
                float bs = 0.f, bp = 0.f;
#pragma unroll
                for (int t = 0; t < BT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = __builtin_amdgcn_exp2f(st[t][r] * scale_log2e - mns);
                        bs += e;
                        bp += e * dp[t][r];
                    }
                l = l * alpha + bs;
                pd = pd * alpha + bp;
                if (j == NB - 1) {
                    l = quad_sum(l);
                    pd = quad_sum(pd);
                    // lse = m c + log2(l) so that P = exp2(s c - lse) needs no multiply by 1/l; D_q / 8 for phase B (attention_bwd.hip)
                    lse = m * scale_log2e + __builtin_amdgcn_logf(l);
                    Dq = pd / l;
                    if (fq == 0 && qvalid) stat[q] = f32x2{lse, 0.125f * Dq};
                }
            } else {
                // dS^T = 0.125 P^T o (dP^T - D_q) as the bf16 B operand; dQ^T += K^T dS^T
#pragma unroll
                for (int u = 0; u < BU; ++u) {
                    PF pf;
                    float ds[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int t = 2 * u + (i >> 2), r = i & 3;
                        const float p = __builtin_amdgcn_exp2f(st[t][r] * scale_log2e - lse);   // masked keys: exp2(-huge) = 0
                        ds[i] = 0.125f * p * (dp[t][r] - Dq);
                    }
                    pf.u[0] = pack_bf16x2(ds[0], ds[1]);
                    pf.u[1] = pack_bf16x2(ds[2], ds[3]);
                    pf.u[2] = pack_bf16x2(ds[4], ds[5]);
                    pf.u[3] = pack_bf16x2(ds[6], ds[7]);
                    VF kf[4];
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        kf[dt].h[0] = tr_read(Ks + u * 4096 + toff[dt]);
                        kf[dt].h[1] = tr_read(Ks + u * 4096 + 2048 + toff[dt]);
                    }
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) o[dt] = mma_acc(kf[dt], pf, o[dt]);
                }
                if (j == NB - 1 && qvalid) {
                    bf16_t *op = obase + (size_t)q * ld + fq * 4;   // dQ[q][dt*16 + 4*fq + r]
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        uint2 wv;
                        wv.x = pack_bf16x2(o[dt][0], o[dt][1]);
                        wv.y = pack_bf16x2(o[dt][2], o[dt][3]);
                        *(uint2 *)(op + dt * 16) = wv;
                    }
                }
            }
        }
    }
    __syncthreads();   // every wave is done with the K / V stages; the statistics are complete

    // ================================ phase B: per key tile -> dK, dV ========================================================
    {
        stage_block(base, ld, gbase, D, 0, ntok, smem, wid, lane);   // Q and dO take the place of K and V
        bf16x8 k0 = {}, k1 = {}, v0 = {}, v1 = {};
        f32x4 dkt[4], dvt[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dkt[dt] = dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        int key = 0;
        bool kvalid = false, edge_tile = false;
        const int total = NC * NB;
        int kc = 0, j = 0;   // step = kc * NB + j
        for (int step = 0; step < total; ++step) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (step + 1 < total) {
                const int nb = j + 1 >= NB ? 0 : j + 1;
                stage_block(base, ld, gbase, D, nb * BK, ntok, smem + ((step + 1) & 1) * STAGE_BYTES, wid, lane);
            }
            const int kt = kc * NW + wid, cj = j;
            if (++j == NB) {
                j = 0;
                ++kc;
            }
            if (kt >= QT) continue;   // wave-uniform
            if (cj == 0) {
                key = kt * 16 + fr;
                kvalid = key < ntok;
                edge_tile = kt * 16 + 16 > ntok;
                row_frag(base + D, ld, kt, k0, k1);
                row_frag(base + 2 * D, ld, kt, v0, v1);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) dkt[dt] = dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const char *Qs = smem + (step & 1) * STAGE_BYTES, *Gs = Qs + BK * 128;
#pragma unroll
            for (int t = 0; t < BT; ++t) {
                const int qt = cj * BT + t;
                // bwd_key_tile_step of attention_tile.h (the resident kernel's call), written out: through the helper the EXT instance's
                // spill deepens from 24 to 28 bytes per lane (profiles/attention_tile_registers.txt)
                if (qt < QT) {   // wave-uniform: tiles past the sequence carry no weight
                    const bf16x8 qf0 = *(const bf16x8 *)(Qs + t * 2048 + off0), qf1 = *(const bf16x8 *)(Qs + t * 2048 + off1);
                    const bf16x8 gf0 = *(const bf16x8 *)(Gs + t * 2048 + off0), gf1 = *(const bf16x8 *)(Gs + t * 2048 + off1);
                    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, d4 = {0.f, 0.f, 0.f, 0.f};
                    s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf0, k0, s4, 0, 0, 0);  // S[q = qt*16 + 4*fq + r][key fr]
                    s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf1, k1, s4, 0, 0, 0);
                    d4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf0, v0, d4, 0, 0, 0);  // dP, same layout
                    d4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf1, v1, d4, 0, 0, 0);
                    if constexpr (EXT) {
                        if (qt * 16 + 15 >= q_con0 && key >= 1 && key <= npatch) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int qq = qt * 16 + fq * 4 + r;
                                if (qq >= q_con0 && qq < ntok) d4[r] += ext[(size_t)(qq - q_con0) * npatch + key - 1];
                            }
                        }
                    }
                    float p[4], ds[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const f32x2 sv = stat[qt * 16 + fq * 4 + r];   // (lse, D_q / 8); a row past the sequence has lse = 1e30 -> P = 0
                        float pr = __builtin_amdgcn_exp2f(s4[r] * scale_log2e - sv[0]);
                        if (edge_tile && !kvalid) pr = 0.f;
                        p[r] = pr;
                        ds[r] = pr * (d4[r] * 0.125f - sv[1]);
                    }
                    union {
                        v4s v;
                        uint32_t u[2];
                    } pb, sb;
                    pb.u[0] = pack_bf16x2(p[0], p[1]);
                    pb.u[1] = pack_bf16x2(p[2], p[3]);
                    sb.u[0] = pack_bf16x2(ds[0], ds[1]);
                    sb.u[1] = pack_bf16x2(ds[2], ds[3]);
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        const v4s gt = tr_read(Gs + t * 2048 + toff[dt]);  // dO^T[d][q]
                        const v4s qT = tr_read(Qs + t * 2048 + toff[dt]);  // Q^T[d][q]
                        dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(gt, pb.v, dvt[dt], 0, 0, 0);
                        dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qT, sb.v, dkt[dt], 0, 0, 0);
                    }
                }
            }
            if (cj == NB - 1 && kvalid) {
                bf16_t *kp = obase + (size_t)key * ld + D + fq * 4, *vp = kp + D;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    uint2 wk, wv;
                    wk.x = pack_bf16x2(dkt[dt][0], dkt[dt][1]);
                    wk.y = pack_bf16x2(dkt[dt][2], dkt[dt][3]);
                    wv.x = pack_bf16x2(dvt[dt][0], dvt[dt][1]);
                    wv.y = pack_bf16x2(dvt[dt][2], dvt[dt][3]);
                    *(uint2 *)(kp + dt * 16) = wk;
                    *(uint2 *)(vp + dt * 16) = wv;
                }
            }
        }
    }
}

template <bool TAP, bool COMPACT>
int launch_fwd(const bf16_t *qkv, int B, int ntok, int heads, bf16_t *out, float *cattn, int ncon, int rev, hipStream_t s) {
    const int QT = COMPACT ? (1 + ncon + 15) / 16 : (ntok + 15) / 16;
    CH_LAUNCH((attention_stream_kernel<TAP, COMPACT>), dim3(B * heads, (QT + NW - 1) / NW), dim3(NW * 64), (size_t)2 * STAGE_BYTES, s, qkv, ntok,
              heads, ATTN_SCALE_LOG2E, out, cattn, ncon, rev);
    CH_LAUNCH_CHECK();
    return 0;
}

std::atomic<int64_t> g_attn_counts[4];

}  // namespace

void ch_attention_count_launch(int which) { g_attn_counts[which & 3].fetch_add(1, std::memory_order_relaxed); }
extern "C" int64_t ch_debug_attention_dispatch_count(int32_t which) {
    return which >= 0 && which < 4 ? g_attn_counts[which].load(std::memory_order_relaxed) : -1;
}

int ch_attention_stream(const bf16_t *qkv, int B, int ntok, int heads, bf16_t *out, hipStream_t s, float *cattn, int ncon, bool compact,
                        bool rev) {
    CH_REQUIRE(ntok <= CH_ATTN_MAX_TOKENS, "attention: more than 1089 tokens per image (a 32 x 32 patch grid) is not supported");
    CH_REQUIRE((int64_t)B * heads <= 0x7fffffff, "attention: batch too large");
    CH_REQUIRE(!cattn || (ncon >= 1 && ncon < ntok - 1), "attention: the concept-attention tap needs 1 <= ncon < ntok - 1");
    const int r = rev ? 1 : 0;
    return ch_attn_pick_mode(cattn != nullptr, compact, [&](auto tap, auto cmp) {
        return launch_fwd<decltype(tap)::value, decltype(cmp)::value>(qkv, B, ntok, heads, out, cattn, ncon, r, s);
    });
}

int ch_attention_bwd_stream(const bf16_t *qkv, const bf16_t *dO, int B, int ntok, int heads, bf16_t *dqkv, hipStream_t s, const float *dpext,
                            int ncon) {
    CH_REQUIRE(ntok <= CH_ATTN_MAX_TOKENS, "attention backward: more than 1089 tokens per image (a 32 x 32 patch grid) is not supported");
    const int NB = (ntok + BK - 1) / BK;
    const size_t lds = (size_t)2 * STAGE_BYTES + (size_t)NB * BK * sizeof(f32x2);   // <= 41.5 KB: under the 64 KB a launch gets unasked
    if (dpext)
        hipLaunchKernelGGL((attention_bwd_stream_kernel<true>), dim3(B * heads), dim3(NW * 64), lds, s, qkv, dO, ntok, heads, ATTN_SCALE_LOG2E, dqkv,
                           dpext, ncon);
    else
        hipLaunchKernelGGL((attention_bwd_stream_kernel<false>), dim3(B * heads), dim3(NW * 64), lds, s, qkv, dO, ntok, heads, ATTN_SCALE_LOG2E, dqkv,
                           (const float *)nullptr, 0);
    CH_LAUNCH_CHECK();
    return 0;
}
