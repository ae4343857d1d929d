// The tile vocabulary of the four attention kernels (attention.hip, attention_bwd.hip, attention_stream.hip): head_dim 64,
// 8 waves per workgroup, 16-row tiles.  The resident and the streaming kernels differ only in how they WALK the sequence; the
// LDS image, the lane geometry that reads it, and every per-tile step are defined here, once.
//
// LDS image of a [rows][64] bf16 matrix: rows of 128 B = eight 16-B chunks, logical chunk c of row r stored at chunk position
// c ^ (r & 7) (img_chunk / img_off).  Three consumers must agree on that rule and all three go through img_chunk:
//   * stage_rows     the LDS-DMA writes lane L's 16 bytes at byte 16 L of the instruction's 1 KB (8 rows), so the swizzle is
//                    applied on the per-lane SOURCE address: lane L fetches logical chunk img_chunk(L >> 3, L & 7);
//   * frag_off       ds_read_b128 of row fr, logical chunks fq and 4 + fq: conflict free;
//   * tr_off         the hardware transpose read ds_read_b64_tr_b16 (a 16-lane group fetches 4 rows x 16 features and each lane
//                    receives one feature column): conflict free with the same swizzle.
// Everything is __device__ __forceinline__ or constexpr; helpers take register arrays by reference and tile indices as
// unrolled constants, so that nothing moves to scratch.  Many instances sit on the 128-VGPR cap of four waves per SIMD, where
// register allocation reacts to spelling: profiles/attention_tile_registers.txt holds every instance's resources against the
// hand-copied kernels and names the fragments that stayed written out.
#pragma once
#include "ch_common.h"

namespace {

constexpr int HD = 64;
constexpr int NW = 8;  // waves per workgroup: 13 query tiles (201 tokens) take two rounds instead of four with 4 waves; K/V staged once
// cache policy of the K / V / Q reads (each element is read exactly once): aux 2 (nt) measured, no gain
// (profiles/r03_cache_policy_ab.txt) -> default policy
constexpr int QKV_AUX = 0;
constexpr float ATTN_SCALE_LOG2E = 0.125f * 1.4426950408889634f;  // head_dim^-0.5 * log2(e), head_dim = 64
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;
typedef float f32x2 __attribute__((ext_vector_type(2)));

union VF {  // A operand assembled from two transpose reads
    bf16x8 v;
    v4s h[2];
};
union PF {  // B operand packed from eight fp32 values
    bf16x8 v;
    uint32_t u[4];
};
struct Frag2 {  // one row's 64 features as held by the four lanes (row, fq = 0..3): columns 8 fq .. and 32 + 8 fq ..
    bf16x8 lo, hi;
};

// ---- the LDS image ---------------------------------------------------------------------------------------------------------
constexpr int ROW_BYTES = 128, TILE_BYTES = 16 * ROW_BYTES, UNIT_BYTES = 32 * ROW_BYTES;
constexpr int img_chunk(int row, int chunk) { return chunk ^ (row & 7); }   // logical <-> stored position: an involution
constexpr int img_off(int row, int chunk) { return row * ROW_BYTES + (img_chunk(row, chunk) << 4); }

// rows [r0, r0 + nrows) of two 64-column blocks of row-major bf16 matrices (matrix, leading dimension, first column) -> the images
// ia and ib; instruction i covers rows 8i .. 8i + 7 (1 KB); rows past the sequence re-read the last row (finite data; masked /
// zero weight downstream)
__device__ __forceinline__ void stage_rows(const bf16_t *a, size_t lda, int cola, const bf16_t *b, size_t ldb, int colb, int r0, int nrows,
                                           int ntok, char *ia, char *ib, int wid, int lane) {
    const int lrow = lane >> 3;
    const int src_chunk = img_chunk(lrow, lane & 7);
    for (int i = wid; i < nrows / 8; i += NW) {
        int row = r0 + i * 8 + lrow;
        row = row < ntok ? row : ntok - 1;
        __builtin_amdgcn_global_load_lds((gbl_void_t *)(a + (size_t)row * lda + src_chunk * 8 + cola), (lds_void_t *)(ia + i * 1024), 16, 0, QKV_AUX);
        __builtin_amdgcn_global_load_lds((gbl_void_t *)(b + (size_t)row * ldb + src_chunk * 8 + colb), (lds_void_t *)(ib + i * 1024), 16, 0, QKV_AUX);
    }
}

// ---- lane geometry ---------------------------------------------------------------------------------------------------------
// b128 fragment of row fr of a tile: features 8 fq .. (half 0) and 32 + 8 fq .. (half 1)
constexpr int frag_off(int fr, int fq, int half) { return img_off(fr, 4 * half + fq); }
// transpose read: lane 4 tq + tp of group fq addresses row 4 fq + tq of a 16-row tile, features 4 tp .. 4 tp + 3 of the
// 16-feature tile dt: chunk = 2 dt + (tp >> 1), half = tp & 1.  (row & 7) of the rows a lane addresses is lane-constant
// (the trow7 = ((fq & 1) << 2) | tq of earlier versions): tiles start at multiples of 16 rows
constexpr int tr_off(int fr, int fq, int dt) {
    const int tq = fr >> 2, tp = fr & 3;
    return img_off(fq * 4 + tq, dt * 2 + (tp >> 1)) + (tp & 1) * 8;
}
struct Lane {
    int fr, fq;      // MFMA fragment row (lane & 15) and quarter (lane >> 4)
    int off0, off1;  // frag_off, both halves
    int toff[4];     // tr_off per 16-feature tile
    __device__ __forceinline__ explicit Lane(int lane) : fr(lane & 15), fq(lane >> 4) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) toff[dt] = tr_off(fr, fq, dt);
        off0 = frag_off(fr, fq, 0);
        off1 = frag_off(fr, fq, 1);
    }
};

// ---- fragments straight from global memory ------------------------------------------------------------------------------------
__device__ __forceinline__ Frag2 ld_frag(const bf16_t *mat, size_t ldm, int row, int fq) {
    return Frag2{*(const bf16x8 *)(mat + (size_t)row * ldm + fq * 8), *(const bf16x8 *)(mat + (size_t)row * ldm + fq * 8 + 32)};
}
// the lane's fragments of `row`, clamped to the last row (rows past the sequence: finite, masked / zero weight)
__device__ __forceinline__ Frag2 row_frag(const bf16_t *mat, size_t ldm, int row, int ntok, int fq) {
    return ld_frag(mat, ldm, min(row, ntok - 1), fq);
}
// query slot j of an image -> (token row, valid); COMPACT: slot 0 = CLS, slots 1.. = the concept tokens (the last ncon rows).
// The row is always inside the sequence, so the forward kernels read it with ld_frag
template <bool COMPACT>
__device__ __forceinline__ int query_slot(int j, int ntok, int ncon, int nqc, bool &valid) {
    if constexpr (COMPACT) {
        valid = j < nqc;
        return !valid ? ntok - 1 : (j == 0 ? 0 : ntok - ncon + j - 1);
    } else {
        valid = j < ntok;
        return valid ? j : ntok - 1;
    }
}

// ---- tile primitives ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Frag2 tile_frag(const char *img, int t, int off0, int off1) {
    return Frag2{*(const bf16x8 *)(img + t * TILE_BYTES + off0), *(const bf16x8 *)(img + t * TILE_BYTES + off1)};
}
// 16 x 16 product over the 64 features: C[row 4 fq + r of a][row fr of b]
__device__ __forceinline__ f32x4 mma2(const Frag2 &a, const Frag2 &b) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.lo, b.lo, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.hi, c, 0, 0, 0);
    return c;
}
__device__ __forceinline__ f32x4 tile_mma(const char *img, int t, int off0, int off1, const Frag2 &b) {
    return mma2(tile_frag(img, t, off0, off1), b);
}
// scores of the keys past the sequence -> -1e30 (the tile's first key is key0)
__device__ __forceinline__ f32x4 mask_tail(f32x4 s, int key0, int ntok, int fq) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (key0 + fq * 4 + r >= ntok) s[r] = -1e30f;
    return s;
}
// a query's keys are spread over the four lanes (fr, fq = 0..3): two cross-lane steps finish a reduction
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
// eight values of one query -> the bf16 B operand of a 32-key unit: logical k = 8 fq + i  <->  key 32 u + (i < 4 ? 4 fq + i : 16 + 4 fq + i - 4)
__device__ __forceinline__ PF pack8(const f32x4 &a, const f32x4 &b) {
    PF pf;
    pf.u[0] = pack_bf16x2(a[0], a[1]);
    pf.u[1] = pack_bf16x2(a[2], a[3]);
    pf.u[2] = pack_bf16x2(b[0], b[1]);
    pf.u[3] = pack_bf16x2(b[2], b[3]);
    return pf;
}
__device__ __forceinline__ v4s tr_read(const char *p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s *)p); }
// the transposed A operand of 32-row unit u: rows 32 u + 4 fq + 0..3 (elements 0..3) and + 16 (elements 4..7), immediate
// offsets off one lane base.  (Arrays passed by reference change how the compiler splits them into registers: where that moved
// an instance's resources, a kernel keeps the dt loop and calls tr_read / mma_acc per tile.)
__device__ __forceinline__ void tr_unit(const char *img, int u, const int (&toff)[4], VF (&vf)[4]) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        vf[dt].h[0] = tr_read(img + u * UNIT_BYTES + toff[dt]);
        vf[dt].h[1] = tr_read(img + u * UNIT_BYTES + TILE_BYTES + toff[dt]);
    }
}
// o^T[feature dt*16 + 4 fq + r][query fr] += (unit^T) (pf)
__device__ __forceinline__ f32x4 mma_acc(const VF &a, const PF &b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0); }
__device__ __forceinline__ void unit_mma(f32x4 (&o)[4], const VF (&vf)[4], const PF &pf) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = mma_acc(vf[dt], pf, o[dt]);
}
// four consecutive features as one 8-byte bf16 store
__device__ __forceinline__ void store_o4(bf16_t *op, const f32x4 v) {
    uint2 w;
    w.x = pack_bf16x2(v[0], v[1]);
    w.y = pack_bf16x2(v[2], v[3]);
    *(uint2 *)op = w;
}
// a lane's 4 x 4 consecutive features of one row as four such stores; op points at feature 4 fq of the row
__device__ __forceinline__ void store_o(bf16_t *op, const f32x4 (&o)[4]) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_o4(op + dt * 16, o[dt]);
}
__device__ __forceinline__ void store_o(bf16_t *op, const f32x4 (&o)[4], float scale) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_o4(op + dt * 16, o[dt] * scale);
}

// ---- the cotangent on the probabilities (EXT): rows q_con0 .. ntok - 1 over keys 1 .. npatch ------------------------------------
struct ExtGrad {
    const float *ext;   // this (image, head)'s [ncon][npatch] block
    int npatch, q_con0;
};
// phase B layout (a lane holds one key's queries qt*16 + 4 fq + r)
__device__ __forceinline__ f32x4 ext_add_col(f32x4 d, const ExtGrad &e, int qt, int key, int ntok, int fq) {
    if (qt * 16 + 15 >= e.q_con0 && key >= 1 && key <= e.npatch) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qq = qt * 16 + fq * 4 + r;
            if (qq >= e.q_con0 && qq < ntok) d[r] += e.ext[(size_t)(qq - e.q_con0) * e.npatch + key - 1];
        }
    }
    return d;
}

// ---- the backward's phase-B step of one (query tile, key tile) -------------------------------------------------------------------
// Q and dO tile t of the images Qs / Gs are queries qt*16 ..; kf / vf are the key tile's K / V fragments (key = the lane's key).
// S = Q K^T and dP = dO V^T in the TRANSPOSED lane layout (a lane holds one key's queries), P and dS rebuilt from the saved
// (lse, D_q / 8) = stat[query] (Stat: f32x4 or f32x2 per query), dV^T += dO^T P and dK^T += Q^T dS by v_mfma_f32_16x16x16_bf16,
// whose reduction index is the 16 queries of the tile: P / dS in the accumulator layout ARE its B operand.
// dead_key: the lane's key is past the sequence (only in the tile that straddles its end)
template <bool EXT, typename Stat>
__device__ __forceinline__ void bwd_key_tile_step(const char *Qs, const char *Gs, int t, int qt, const Frag2 &kf, const Frag2 &vf,
                                                  const Stat *stat, float scale_log2e, int key, bool dead_key, int ntok, const ExtGrad &e,
                                                  int off0, int off1, const int (&toff)[4], int fq, f32x4 (&dkt)[4], f32x4 (&dvt)[4]) {
    const Frag2 qf = tile_frag(Qs, t, off0, off1), gf = tile_frag(Gs, t, off0, off1);
    const f32x4 s4 = mma2(qf, kf);   // S[q = qt*16 + 4*fq + r][key fr]
    f32x4 d4 = mma2(gf, vf);         // dP, same layout
    if constexpr (EXT) d4 = ext_add_col(d4, e, qt, key, ntok, fq);
    float p[4], ds[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const Stat sv = stat[qt * 16 + fq * 4 + r];
        float pr = __builtin_amdgcn_exp2f(s4[r] * scale_log2e - sv[0]);
        if (dead_key) pr = 0.f;
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
        const v4s gt = tr_read(Gs + t * TILE_BYTES + toff[dt]);  // dO^T[d][q]
        const v4s qT = tr_read(Qs + t * TILE_BYTES + toff[dt]);  // Q^T[d][q]
        dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(gt, pb.v, dvt[dt], 0, 0, 0);
        dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qT, sb.v, dkt[dt], 0, 0, 0);
    }
}

}  // namespace
