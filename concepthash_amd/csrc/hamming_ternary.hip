// Ternary codes (gfx950): pack, distance matrix, exact top-k and the rank-counting evaluation, all integers, so any segmentation or
// sharding of the gallery gives the same bits ("ternary codes").
//
// The ternary code of a real code x: t_j = sign(x_j) where |x_j| > margin, 0 otherwise (NaN -> 0: the comparison is false).  Packed as
// TWO bit planes per row, [rows, 2, W] uint64, adjacent, so a gallery row is one contiguous load of 2 W words:
//     plane 0 (sign)  bit j = t_j > 0            plane 1 (mask)  bit j = t_j != 0            bits past nbit: zero in both
// The distance is K(q, g) = nbit - sum_j t_q,j t_g,j in [0, 2 nbit] ("half bits": a disagreement both sides are sure of costs 2, a bit
// either side is unsure of costs 1, an agreement 0).  With A = popcount(mq & mg) and X = popcount((sq ^ sg) & mq & mg): K = nbit - A + 2 X.
//
// Top-k (ch_ternary_topk) is topk_scan of hamming_shared.h with this distance: one lane per query, its two planes in 4 W VGPRs, the
// gallery row's 2 W words wave-uniform through the scalar load path.  key = K << 22 | row in segment: K <= 512 takes 10 bits (the
// plain scan's shift of 23 leaves 9), so a segment holds at most 2^22 = 4,194,304 rows (checked on the host in topk_run) and the
// largest key, 512 << 22 | 2^22 - 1, stays below the empty slot 0xFFFFFFFF.  ch_ternary_topk_filtered is the same kernel template with
// the TopkFilter of hamming_shared.h (allow-list bitmap, per-query group test) as its Filter argument: one more instance per (W, KREG).
// What the compiler emits per 32-bit word of the top-k distance (disassembly of topk_ternary_partial_kernel, every W and KREG):
//     v_and_b32       t, s[mg], v[mq]            mq & mg
//     v_bcnt_u32_b32  A, t, A                    chained
//     v_bitop3_b32    x, v[sq], s[sg], t         (sq ^ sg) & t, the gallery sign word its one SGPR operand (truth table 0x28)
//     v_bcnt_u32_b32  X, x, X                    chained
// 4 VALU instructions per word, then per row v_sub_u32 (nbit - A, nbit in an SGPR), v_lshl_add_u32 (2 X + that) and the
// v_lshl_or_b32 of make_key -- against 2 per word and the v_lshl_or_b32 for the plain distance.  The last two of the four are one asm
// block (xor_and_bcnt_acc): from C++ the compiler emitted FIVE per word -- it re-associates (sq ^ sg) & (mq & mg) into v_xor_b32 with
// sg plus a three-way-AND v_bitop3_b32 with mg, i.e. it spends the one SGPR operand of the v_bitop3_b32 on the mask word and needs a
// separate instruction for the sign word.  No instance uses scratch; W <= 2 scans blocks of 4 rows, W >= 3 of 2 (two buffers of
// 16 W SGPRs would not fit at 4).  The rank-count scan holds the QUERY's words in SGPRs and compiles to the same four from C++.
//
// The evaluation (ch_ternary_rank_collect / ch_ternary_rank_count) is the collect and count passes of hamming_shared.h -- kernels,
// launches and entry bodies -- under K (TernaryRanking below), with the CSR buffers and the key K << 32 | global index of
// hamming_rankcount.hip; ch_hamming_rank_ap turns the bins into AP integers unchanged.  K does not go through the LDS-histogram passes of hamming.hip: 2 nbit + 1 buckets do not fit their counters at W = 4.
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "hamming_shared.h"

namespace {

constexpr int TKEY_SHIFT = 22;
static_assert((512u << TKEY_SHIFT | ((1u << TKEY_SHIFT) - 1u)) < 0xFFFFFFFFu && (512u << TKEY_SHIFT) >> TKEY_SHIFT == 512u,
              "K <= 2 * 256 and a row of the segment share a 32-bit key below the empty slot");

// ---------------------------------------------------------------------------------------------------------------
// pack: one launch writes both planes
// ---------------------------------------------------------------------------------------------------------------
// thread = one bit; a 64-lane wave = one (row, word): two ballots, lane 0 stores the sign and the mask word
__global__ __launch_bounds__(256) void pack_ternary_kernel(const float *__restrict__ codes, int64_t rows, int nbit, int W, float margin,
                                                           uint64_t *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t word = gid >> 6;
    const int bit = (int)(gid & 63);
    if (word >= rows * W) return;   // wave-uniform
    const int64_t r = word / W;
    const int w = (int)(word - r * W);
    const int i = w * 64 + bit;
    const float x = i < nbit ? codes[r * nbit + i] : 0.f;
    const bool sure = i < nbit && __builtin_fabsf(x) > margin;   // false for NaN
    const uint64_t m = __builtin_amdgcn_ballot_w64(sure);
    const uint64_t s = __builtin_amdgcn_ballot_w64(sure && x > 0.f);
    if (bit == 0) {
        out[(r * 2 + 0) * W + w] = s;
        out[(r * 2 + 1) * W + w] = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the distance, three ways
// ---------------------------------------------------------------------------------------------------------------
// everything read from memory (the distance matrix; the collect pass, for relevant rows only)
__device__ __forceinline__ uint32_t ternary_dist_row(const uint64_t *__restrict__ q, const uint64_t *__restrict__ g, int W, uint32_t nbit) {
    uint32_t a = 0, x = 0;
    for (int w = 0; w < W; ++w) {
        const uint64_t t = q[W + w] & g[W + w];
        a += (uint32_t)__builtin_popcountll(t);
        x += (uint32_t)__builtin_popcountll((q[w] ^ g[w]) & t);
    }
    return nbit - a + 2u * x;
}

// popcount((sq ^ sg) & t) + acc with the gallery's sign word the SGPR operand: v_bitop3_b32 (truth table 0x28 = (a ^ b) & c) and the
// chained v_bcnt, in one asm block.  Written in C++ the compiler re-associates (sq ^ sg) & (mq & mg) into a v_xor_b32 with sg and a
// three-way AND with mg as the v_bitop3_b32's SGPR operand: 5 instructions per word.
__device__ __forceinline__ uint32_t xor_and_bcnt_acc(uint32_t sq, uint32_t sg_uniform, uint32_t t, uint32_t acc) {
    uint32_t d;
    asm("v_bitop3_b32 %0, %2, %3, %4 bitop3:0x28\n\t"
        "v_bcnt_u32_b32 %0, %0, %1"
        : "=&v"(d)
        : "v"(acc), "v"(sq), "s"(sg_uniform), "v"(t));
    return d;
}

// the top-k scan: the query's planes in the lane's VGPRs, the gallery row (sign words, then mask words) wave-uniform
template <int W>
__device__ __forceinline__ uint32_t ternary_dist_lane(const uint32_t (&sq)[2 * W], const uint32_t (&mq)[2 * W], uint32_t nbit,
                                                      const uint64_t *__restrict__ g) {
    uint32_t a = 0, x = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t sg = g[w], mg = g[W + w];
        const uint32_t t0 = mq[2 * w] & (uint32_t)mg, t1 = mq[2 * w + 1] & (uint32_t)(mg >> 32);
        a = bcnt_acc(t0, a);
        x = xor_and_bcnt_acc(sq[2 * w], (uint32_t)sg, t0, x);
        a = bcnt_acc(t1, a);
        x = xor_and_bcnt_acc(sq[2 * w + 1], (uint32_t)(sg >> 32), t1, x);
    }
    return nbit - a + 2u * x;
}

// the rank-count scan: the query's planes wave-uniform, the gallery row the lane's own -- the same four instructions per word, the
// query's sign word the one SGPR operand of the v_bitop3_b32
template <int W>
struct TernaryUniform {
    static constexpr int ROW = 2 * W;
    struct Regs {
        uint32_t sq[2 * W], mq[2 * W], nbit;
        const uint64_t *gp;   // the segment's first row
    };
    const uint64_t *q;
    uint32_t nbit;
    __device__ __forceinline__ void load(Regs &r, int64_t qi, const uint64_t *__restrict__ g, int64_t g0) const {
        r.gp = g + g0 * ROW;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t s = q[qi * 2 * W + w], m = q[qi * 2 * W + W + w];
            r.sq[2 * w] = __builtin_amdgcn_readfirstlane((uint32_t)s);
            r.sq[2 * w + 1] = __builtin_amdgcn_readfirstlane((uint32_t)(s >> 32));
            r.mq[2 * w] = __builtin_amdgcn_readfirstlane((uint32_t)m);
            r.mq[2 * w + 1] = __builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
        }
        r.nbit = nbit;
    }
    __device__ __forceinline__ static uint32_t at(const Regs &r, const uint64_t (&g)[2 * W]) {
        uint32_t a = 0, x = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t t0 = r.mq[2 * w] & (uint32_t)g[W + w], t1 = r.mq[2 * w + 1] & (uint32_t)(g[W + w] >> 32);
            a = bcnt_acc(t0, a);
            x = bcnt_acc((r.sq[2 * w] ^ (uint32_t)g[w]) & t0, x);
            a = bcnt_acc(t1, a);
            x = bcnt_acc((r.sq[2 * w + 1] ^ (uint32_t)(g[w] >> 32)) & t1, x);
        }
        return r.nbit - a + 2u * x;
    }
    __device__ __forceinline__ void rows(const Regs &r, int nrows, uint64_t row0, const uint64_t *list, uint32_t n, uint64_t last,
                                         uint32_t *bins) const {
        rank_count_rows<TernaryUniform>(r, r.gp, nrows, row0, list, n, last, bins);
    }
};

struct TernaryRow {
    const uint64_t *q;
    uint32_t nbit;
    __device__ __forceinline__ uint32_t row(int64_t qi, int W, const uint64_t *__restrict__ g, int64_t j) const {
        return ternary_dist_row(q + qi * 2 * W, g + j * 2 * W, W, nbit);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ternary_dist_kernel(const uint64_t *__restrict__ q, int64_t Qn, const uint64_t *__restrict__ g,
                                                           int64_t G, int W, uint32_t nbit, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= Qn * G) return;
    const int64_t qi = t / G, j = t - qi * G;
    out[t] = (int32_t)ternary_dist_row(q + qi * 2 * W, g + j * 2 * W, W, nbit);
}

// rows of one block of scalar loads: a row is 2 W words = 4 W SGPRs, and two buffers of blocks are in flight
constexpr int ternary_ub(int W) { return W <= 2 ? 4 : 2; }

// Filter: TopkNoFilter (ch_ternary_topk) or TopkFilter (ch_ternary_topk_filtered), hamming_shared.h: one more instance per (W, KREG).
// The key of a row that is not admitted is the empty slot, which the static_assert beside TKEY_SHIFT keeps above every real key.
template <int W, int KREG, class Filter>
__global__ __launch_bounds__(256) void topk_ternary_partial_kernel(const uint64_t *__restrict__ q, int64_t Qn,
                                                                   const uint64_t *__restrict__ g, int64_t G, uint32_t nbit, int seg_rows,
                                                                   int k, uint32_t *__restrict__ part, Filter flt) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t sq[2 * W], mq[2 * W];   // a lane past Qn holds zero planes: K = nbit for every row, and nothing of it is stored
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t s = qi < Qn ? q[qi * 2 * W + w] : 0ull, m = qi < Qn ? q[qi * 2 * W + W + w] : 0ull;
        sq[2 * w] = (uint32_t)s;
        sq[2 * w + 1] = (uint32_t)(s >> 32);
        mq[2 * w] = (uint32_t)m;
        mq[2 * w + 1] = (uint32_t)(m >> 32);
    }
    topk_scan<2 * W, KREG, TKEY_SHIFT, ternary_ub(W)>([&](const uint64_t *gw) { return ternary_dist_lane<W>(sq, mq, nbit, gw); }, qi, Qn, g,
                                                      G, seg_rows, k, part, flt);
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
// VGPRs of topk_ternary_partial_kernel<W, KREG, TopkNoFilter> from the code-object metadata of this build (no instance uses scratch);
// topk_seg_rows_table (hamming_shared.h) turns them into segments
constexpr int TTOPK_VGPRS[4][5] = {
    // KREG 10, 16, 32, 64, 128
    {26, 38, 70, 134, 258}, {30, 42, 74, 138, 258}, {34, 46, 78, 142, 258}, {38, 50, 82, 146, 258},   // W = 1..4
};

// ... and of topk_ternary_partial_kernel<W, KREG, TopkFilter> (profiles/search_filtered_topk.txt): its segments follow its own figures
constexpr int FTTOPK_VGPRS[4][5] = {
    {30, 41, 73, 136, 259}, {35, 47, 79, 141, 259}, {41, 53, 85, 147, 260}, {45, 57, 89, 151, 260},   // W = 1..4
};

int ttopk_seg_rows(int64_t Qn, int64_t G, int W, int k, bool filtered) {
    return topk_seg_rows_table(Qn, G, (filtered ? FTTOPK_VGPRS : TTOPK_VGPRS)[W - 1][topk_list_index(k)], (int64_t)1 << TKEY_SHIFT);
}

size_t ttopk_workspace(int64_t Qn, int64_t G, int W, int k, bool filtered) {
    if (W < 1 || W > 4) return 16;
    return topk_workspace_bytes(Qn, G, k, [&] { return ttopk_seg_rows(Qn, G, W, k, filtered); });
}

struct TernaryScan {
    static constexpr int SHIFT = TKEY_SHIFT;
    static constexpr const char *too_many_segments = "ternary_topk: gallery too large for one call: more than 65,535 segments (shard it)";
    int nbit;
    int check(int W) const {
        CH_REQUIRE(nbit >= 1 && nbit <= 64 * W, "ternary_topk: nbit must be in [1, 64 W]");
        return 0;
    }
    bool operands() const { return true; }
    int seg_rows(int64_t Qn, int64_t G, int W, int k, bool filtered) const { return ttopk_seg_rows(Qn, G, W, k, filtered); }
    size_t workspace(int64_t Qn, int64_t G, int W, int k, bool filtered) const { return ttopk_workspace(Qn, G, W, k, filtered); }
    template <int W, int KREG, class Filter>
    void launch(const TopkCall &c, const Filter &flt) const {
        hipLaunchKernelGGL((topk_ternary_partial_kernel<W, KREG, Filter>), c.grid, dim3(256), 0, c.s, c.q, c.Qn, c.g, c.G, (uint32_t)nbit,
                           c.seg_rows, c.k, c.part, flt);
    }
};

// what rank_collect_run / rank_count_run (hamming_shared.h) take as the ranking
struct TernaryRanking {
    static constexpr const char *with_offsets = "q and keys";
    const uint64_t *q;
    int W, nbit;
    int check(const char *who, int64_t Qn, int64_t G, int64_t g_index_base) const {
        if (int e = check_rank_sizes(who, Qn, G, W, g_index_base)) return e;
        CH_REQUIRE(nbit >= 1 && nbit <= 64 * W, std::string(who) + ": nbit must be in [1, 64 W]");
        return 0;
    }
    bool operands() const { return q != nullptr; }
    template <class F> int collect(F &&f) const { return f(TernaryRow{q, (uint32_t)nbit}, W); }
    template <class F>
    int count(F &&f) const {
        return dispatch_w(W, [&](auto w) { return f(TernaryUniform<decltype(w)::value>{q, (uint32_t)nbit}); });
    }
};

}  // namespace

extern "C" int ch_pack_ternary(const float *codes, int64_t rows, int32_t nbit, float margin, uint64_t *out_planes, void *stream) {
    CH_REQUIRE(nbit >= 1 && nbit <= 256, "pack_ternary: nbit must be in [1, 256]");
    CH_REQUIRE(std::isfinite(margin) && margin >= 0.f, "pack_ternary: margin must be finite and >= 0");
    CH_REQUIRE(rows >= 0, "pack_ternary: negative rows");
    if (rows == 0) return 0;
    CH_REQUIRE(codes && out_planes, "pack_ternary: null pointer");
    const int W = (nbit + 63) / 64;
    hipLaunchKernelGGL(pack_ternary_kernel, dim3((unsigned)ceil_div64(rows * W * 64, 256)), dim3(256), 0, (hipStream_t)stream, codes, rows,
                       (int)nbit, W, margin, out_planes);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_ternary_dist(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, int32_t *out,
                               void *stream) {
    CH_REQUIRE(W >= 1 && W <= 4, "ternary_dist: 1 <= W <= 4 (nbit <= 256)");
    CH_REQUIRE(nbit >= 1 && nbit <= 64 * W, "ternary_dist: nbit must be in [1, 64 W]");
    CH_REQUIRE(Qn >= 0 && G >= 0, "ternary_dist: negative sizes");
    if (Qn == 0 || G == 0) return 0;
    CH_REQUIRE(q && g && out, "ternary_dist: null pointer");
    hipLaunchKernelGGL(ternary_dist_kernel, dim3((unsigned)ceil_div64(Qn * G, 256)), dim3(256), 0, (hipStream_t)stream, q, Qn, g, G, (int)W,
                       (uint32_t)nbit, out);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ch_ternary_topk_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k) {
    return ttopk_workspace(Qn, G, W, k, false);
}

extern "C" int ch_ternary_topk(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, int32_t k,
                               int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *workspace, size_t workspace_bytes,
                               void *stream) {
    return topk_run("ternary_topk", TernaryScan{(int)nbit}, q, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace, workspace_bytes,
                    (hipStream_t)stream, TopkNoFilter{});
}

extern "C" size_t ch_ternary_topk_filtered_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k) {
    return ttopk_workspace(Qn, G, W, k, true);
}

extern "C" int ch_ternary_topk_filtered(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, int32_t k,
                                        int64_t g_index_base, const uint64_t *allow, const int32_t *group, const int64_t *want,
                                        int32_t exclude, int64_t *out_idx, int32_t *out_dist, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    return topk_run("ternary_topk_filtered", TernaryScan{(int)nbit}, q, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace,
                    workspace_bytes, (hipStream_t)stream, TopkFilter{allow, group, want, g_index_base, (int)exclude});
}

extern "C" int ch_ternary_rank_collect(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit,
                                       const void *q_labels, const void *g_labels, int32_t LW, int64_t g_index_base, const int64_t *offsets,
                                       uint32_t *count, uint64_t *keys, void *stream) {
    return rank_collect_run("ternary_rank_collect", TernaryRanking{q, (int)W, (int)nbit}, Qn, g, G, q_labels, g_labels, (int)LW, g_index_base,
                            offsets, count, keys, (hipStream_t)stream);
}

extern "C" int ch_ternary_rank_count(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit,
                                     int64_t g_index_base, int32_t seg_rows, const int64_t *offsets, const uint64_t *keys,
                                     int32_t list_cap, uint32_t *bins, void *stream) {
    return rank_count_run("ternary_rank_count", TernaryRanking{q, (int)W, (int)nbit}, Qn, g, G, g_index_base, (int)seg_rows, offsets, keys,
                          (int)list_cap, bins, (hipStream_t)stream);
}
