// Exact top-k search on packed codes (gfx950) under three distances, all integers, so any segmentation or sharding of the gallery
// gives the same bits:
//     plain     popcount(q ^ g)                                                    ch_hamming_topk
//     masked    popcount((q ^ g) & mask), the query's own mask or one for all      ch_hamming_topk_masked
//     weighted  sum_j w_ij [bit_j(q_i) != bit_j(g)] = sum_p 2^p popcount((q_i ^ g) & planes[i, p]): the gallery stays binary, the query
//               pays w_j for a disagreement on bit j, with w_j its own |code_j| quantised to P = 4 or 8 bits and planes[i, p] = bit p of
//               every w_ij ("weighted distance")            ch_weight_planes, ch_hamming_topk_weighted
//
// ONE scan (topk_scan, hamming_shared.h, which the ternary distance of hamming_ternary.hip takes too) serves the three: one LANE per QUERY (its code words, its mask or plane words and its list live in that lane's
// registers), the GALLERY segment is walked sequentially and is wave-uniform, so gallery words arrive through the scalar data path
// (s_load_dwordx{4,8,16}) and every XOR uses an SGPR operand.  Nothing of size Qn x G is ever written.  grid = (query tiles, gallery
// segments) so small galleries still fill the chip.  Per lane a sorted list of the KREG smallest keys, key = dist << SHIFT |
// row-in-segment (unique, so "k smallest keys" == ascending (distance, gallery index)).  A wave-uniform branch skips the insertion
// network unless some lane beats its current threshold; the network itself is branch free (min/max chain).
//     SHIFT = 23 (plain, masked): dist <= 256, segments of < 2^23 rows.
//     SHIFT = 16 (weighted): D <= 255 * 256 = 65,280 < 2^16 - 1, so 0xFFFFFFFF stays the empty slot; segments hold <= 65,536 rows.
// Filtered search (ch_hamming_topk_filtered, ch_hamming_topk_weighted_filtered): the same scans with the TopkFilter of hamming_shared.h --
// an allow-list bitmap on the scalar path and a per-query group test -- as the Filter argument of the one kernel template per distance,
// topk_partial_kernel<W, KREG, MASKED, Filter> and topk_weighted_partial_kernel<W, KREG, P, Filter>: one more instance per
// (W, KREG, MASKED) and (W, KREG, P), and TopkNoFilter, an empty argument, for the unfiltered ones.  A row that is not admitted gets
// the empty-slot key 0xFFFFFFFF, which the static_asserts below keep above every real key.
// topk_merge_keys_kernel<SHIFT> merges the per-segment lists of a call, topk_merge_lists_kernel the final lists of several shards;
// subcode_dist_kernel breaks the distance of retrieved hits down by concept.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "hamming_shared.h"

namespace {

constexpr int KEY_SHIFT = 23;
constexpr int WKEY_SHIFT = 16;
// the empty slot -- also the key of a row a filter does not admit -- is above every real key: the largest distance with the last row
// of the longest segment (topk_seg_rows: < 2^23 rows; wtopk_seg_rows: <= 2^16)
static_assert((256u << KEY_SHIFT | ((1u << KEY_SHIFT) - 2u)) < 0xFFFFFFFFu && (256u << KEY_SHIFT) >> KEY_SHIFT == 256u,
              "dist <= 256 and a row of the segment share a 32-bit key below the empty slot");
static_assert((65280u << WKEY_SHIFT | ((1u << WKEY_SHIFT) - 1u)) < 0xFFFFFFFFu && (65280u << WKEY_SHIFT) >> WKEY_SHIFT == 65280u,
              "D <= 255 * 256 and a row of the segment share a 32-bit key below the empty slot");

// ---------------------------------------------------------------------------------------------------------------
// the three distances of one gallery row (bcnt_acc, load_query and the plain hamming<W>: hamming_shared.h)
// ---------------------------------------------------------------------------------------------------------------
// popcount((q ^ g) & m): the mask words sit in the lane's VGPRs beside its query words, so a masked distance costs one v_and per
// 32-bit word in front of the chained v_bcnt -- 3 instructions per word (ch_hamming_topk_masked)
template <int W>
__device__ __forceinline__ int hamming_masked(const uint32_t (&q)[2 * W], const uint32_t (&m)[2 * W], const uint64_t *__restrict__ g) {
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t gw = g[w];
        d = bcnt_acc((q[2 * w] ^ (uint32_t)gw) & m[2 * w], d);
        d = bcnt_acc((q[2 * w + 1] ^ (uint32_t)(gw >> 32)) & m[2 * w + 1], d);
    }
    return (int)d;
}

// horner2, sum_p 2^p a[p] as one block of P - 1 v_lshl_add_u32: hamming_shared.h
// weighted D: per 32-bit word and plane one (q ^ g) & plane (a single v_bitop3_b32 with the gallery word as its SGPR operand) and one
// chained v_bcnt into that plane's accumulator -- 2 P instructions per word -- then the Horner chain of P - 1 shift-adds
template <int W, int P>
__device__ __forceinline__ uint32_t weighted_dist(const uint32_t (&q)[2 * W], const uint32_t (&pl)[P][2 * W],
                                                  const uint64_t *__restrict__ g) {
    uint32_t acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t gw = g[w];
        const uint32_t lo = (uint32_t)gw, hi = (uint32_t)(gw >> 32);
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = bcnt_acc((q[2 * w] ^ lo) & pl[p][2 * w], acc[p]);
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = bcnt_acc((q[2 * w + 1] ^ hi) & pl[p][2 * w + 1], acc[p]);
    }
    return horner2(acc);
}

// MASKED (ch_hamming_topk_masked): the query's own mask -- row qi of a [Qn, W] array (stride W) -- or one mask shared by all queries
// (stride 0).  The unmasked instantiations carry an empty argument and no mask code.
template <bool MASKED>
struct TopkMask {};
template <>
struct TopkMask<true> {
    const uint64_t *mask;
    int stride;
};

// Filter: TopkNoFilter (ch_hamming_topk, ch_hamming_topk_masked) or TopkFilter (ch_hamming_topk_filtered), hamming_shared.h: one more
// instance per (W, KREG, MASKED), every part of the filter a run-time condition of it
template <int W, int KREG, bool MASKED, class Filter>
__global__ __launch_bounds__(256) void topk_partial_kernel(const uint64_t *__restrict__ q, int64_t Qn,
                                                           const uint64_t *__restrict__ g, int64_t G, int seg_rows, int k,
                                                           uint32_t *__restrict__ part, TopkMask<MASKED> qm, Filter flt) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t qw[2 * W];
    load_query<W>(qw, q, qi, Qn);
    if constexpr (MASKED) {
        uint32_t mw[2 * W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t v = qi < Qn ? qm.mask[qi * qm.stride + w] : 0ull;
            mw[2 * w] = (uint32_t)v;
            mw[2 * w + 1] = (uint32_t)(v >> 32);
        }
        topk_scan<W, KREG, KEY_SHIFT>([&](const uint64_t *gw) { return (uint32_t)hamming_masked<W>(qw, mw, gw); }, qi, Qn, g, G, seg_rows, k,
                                      part, flt);
    } else {
        topk_scan<W, KREG, KEY_SHIFT>([&](const uint64_t *gw) { return (uint32_t)hamming<W>(qw, gw); }, qi, Qn, g, G, seg_rows, k, part,
                                      flt);
    }
}

// Filter: TopkNoFilter (ch_hamming_topk_weighted) or TopkFilter (ch_hamming_topk_weighted_filtered)
template <int W, int KREG, int P, class Filter>
__global__ __launch_bounds__(256) void topk_weighted_partial_kernel(const uint64_t *__restrict__ q,
                                                                    const uint64_t *__restrict__ planes, int64_t Qn,
                                                                    const uint64_t *__restrict__ g, int64_t G, int seg_rows, int k,
                                                                    uint32_t *__restrict__ part, Filter flt) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t qw[2 * W];
    load_query<W>(qw, q, qi, Qn);
    uint32_t pl[P][2 * W];   // a lane past Qn holds zero planes: its distances are 0 and nothing of it is stored
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t v = qi < Qn ? planes[(qi * P + p) * W + w] : 0ull;
            pl[p][2 * w] = (uint32_t)v;
            pl[p][2 * w + 1] = (uint32_t)(v >> 32);
        }
    }
    topk_scan<W, KREG, WKEY_SHIFT>([&](const uint64_t *gw) { return weighted_dist<W, P>(qw, pl, gw); }, qi, Qn, g, G, seg_rows, k, part,
                                   flt);
}

// merge already-final lists (idx,dist) from several shards: same extraction on composite (dist, idx)
__global__ __launch_bounds__(256) void topk_merge_lists_kernel(const int64_t *__restrict__ idx_lists,
                                                               const int32_t *__restrict__ dist_lists, int nlists, int64_t Qn,
                                                               int k, int64_t *out_idx, int32_t *out_dist) {
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (qi >= Qn) return;
    const int ncand = nlists * k;
    unsigned long long prev = 0ull;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = ~0ull;
        for (int c = lane; c < ncand; c += 64) {
            const int s = c / k, i = c - s * k;
            const int32_t d = dist_lists[((size_t)s * Qn + qi) * k + i];
            if (d < 0) continue;
            const unsigned long long comp =
                ((unsigned long long)d << 48) | (unsigned long long)idx_lists[((size_t)s * Qn + qi) * k + i];
            if (comp + 1 > prev && comp < best) best = comp;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        if (lane == 0) {
            out_idx[qi * k + r] = best == ~0ull ? -1 : (int64_t)(best & ((1ull << 48) - 1));
            out_dist[qi * k + r] = best == ~0ull ? -1 : (int32_t)(best >> 48);
        }
        if (best != ~0ull) prev = best + 1;
    }
}

// Per-concept breakdown of retrieved hits (ch_hamming_subcode_dist): one thread per (query, hit) gathers the hit's row and counts
// the differing bits inside each of the nsub equal sub-codes of sb = nbit / nsub bits; a sub-code may straddle a 64-bit word.
__global__ __launch_bounds__(256) void subcode_dist_kernel(const uint64_t *__restrict__ q, int64_t Qn, const uint64_t *__restrict__ g,
                                                           int64_t G, int W, const int64_t *__restrict__ idx, int k,
                                                           int64_t g_index_base, int sb, int nsub, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Qn * k) return;
    const int64_t qi = t / k;
    const int64_t row = idx[t] - g_index_base;
    int32_t *o = out + t * nsub;
    if (idx[t] < 0 || row < 0 || row >= G) {   // -1 = no hit; anything else out of range was refused by the host check
        for (int c = 0; c < nsub; ++c) o[c] = -1;
        return;
    }
    const uint64_t *qp = q + qi * W, *gp = g + row * W;
    for (int c = 0; c < nsub; ++c) {
        const int lo = c * sb, hi = lo + sb;
        int d = 0;
        for (int w = lo >> 6; w <= (hi - 1) >> 6; ++w) {
            const int a = max(lo, 64 * w) - 64 * w, nb = min(hi, 64 * w + 64) - 64 * w - a;
            const uint64_t m = (nb == 64 ? ~0ull : ((1ull << nb) - 1ull)) << a;
            d += __builtin_popcountll((qp[w] ^ gp[w]) & m);
        }
        o[c] = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// quantised weights -> bit planes
// ---------------------------------------------------------------------------------------------------------------
// One wave per query; lane b holds bit b of every 64-bit word (W <= 4 values).  a = |c| (0 where c is not finite, the bit is masked
// out or past nbit); amax by wave shuffles; w = floor(a L / amax + 0.5) in fp64 on the widened fp32 values (a L is exact, the IEEE
// quotient and the sum round as the host's do); plane p of word t is the 64-lane ballot of bit p of w.  planes [Qn, P, W]; wsum [Qn] =
// the largest D a query can reach.
template <int P>
__global__ __launch_bounds__(256) void weight_planes_kernel(const float *__restrict__ codes, int64_t Qn, int nbit, int W,
                                                            const uint64_t *__restrict__ mask, int mask_stride,
                                                            uint64_t *__restrict__ planes, int32_t *__restrict__ wsum) {
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (qi >= Qn) return;  // wave-uniform
    constexpr double L = (double)((1 << P) - 1);
    float a[4];
    float amax = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        a[t] = 0.f;
        const int j = 64 * t + lane;
        if (t < W && j < nbit) {
            const uint32_t bits = __builtin_bit_cast(uint32_t, codes[qi * nbit + j]) & 0x7FFFFFFFu;   // |c|
            const bool finite = bits < 0x7F800000u;
            const bool kept = mask == nullptr || ((mask[qi * mask_stride + t] >> lane) & 1ull) != 0ull;
            a[t] = (finite && kept) ? __builtin_bit_cast(float, bits) : 0.f;
        }
        amax = fmaxf(amax, a[t]);
    }
    amax = wave_max(amax);
    uint32_t sum = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint32_t w = 0;
        if (amax > 0.f) w = (uint32_t)__builtin_floor((double)a[t] * L / (double)amax + 0.5);
        sum += w;
        if (t < W) {   // wave-uniform
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const uint64_t plane = __builtin_amdgcn_ballot_w64(((w >> p) & 1u) != 0u);
                if (lane == 0) planes[(qi * P + p) * W + t] = plane;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) wsum[qi] = (int32_t)sum;
}

// ---------------------------------------------------------------------------------------------------------------
// host: segment sizing (topk_seg_rows_for, topk_seg_rows_table, topk_list_index: hamming_shared.h)
// ---------------------------------------------------------------------------------------------------------------
// The scan kernels have no LDS, so residency is set by their registers.  The rule below is the one the plain and masked unfiltered
// scans were tuned and measured with; it is NOT the table form (which gives 6, not 7, workgroups for the plain lists of 32 keys), so
// it stays apart.
// 24-42 VGPRs for lists of <= 16 keys (8 workgroups of four waves per CU), 68-74 for 32 (7), ~136 for 64 (3), the whole file for 128 (1)
constexpr int TOPK_PER_CU[5] = {8, 8, 7, 3, 1};   // by list length (topk_list_index)
int topk_seg_rows(int64_t Qn, int64_t G, int k) {
    return topk_seg_rows_for(Qn, G, TOPK_PER_CU[topk_list_index(k)], (int64_t)(1 << KEY_SHIFT) - 1);
}

// The filtered scans follow their OWN registers (profiles/search_filtered_topk.txt: 1 to 7 VGPRs above their siblings, no scratch),
// in the table form.  It differs from the rule above at lists of 32 keys only (7, 6 or 5 workgroups per CU, not 7 throughout).
// VGPRs of topk_partial_kernel<W, KREG, MASKED, TopkFilter> from the code-object metadata of this build:
constexpr int FTOPK_VGPRS[2][4][5] = {
    // KREG 10, 16, 32, 64, 128
    {{28, 40, 72, 134, 259}, {30, 41, 73, 136, 259}, {33, 45, 77, 139, 259}, {35, 47, 79, 141, 259}},   // plain, W = 1..4
    {{30, 42, 74, 136, 259}, {34, 46, 78, 140, 259}, {39, 51, 83, 145, 259}, {43, 55, 87, 149, 259}},   // masked, W = 1..4
};

int ftopk_seg_rows(int64_t Qn, int64_t G, int W, int k, bool masked) {
    return topk_seg_rows_table(Qn, G, FTOPK_VGPRS[masked][W - 1][topk_list_index(k)], (int64_t)(1 << KEY_SHIFT) - 1);
}

// VGPRs of topk_weighted_partial_kernel<W, KREG, P, TopkNoFilter> from the code-object metadata of this build
// (profiles/search_weighted_topk.txt; no instance uses scratch)
constexpr int WTOPK_VGPRS[2][4][5] = {
    // KREG 10, 16, 32, 64, 128
    {{32, 44, 76, 140, 258}, {43, 54, 86, 150, 258}, {53, 64, 96, 160, 258}, {63, 74, 106, 170, 258}},     // P = 4, W = 1..4
    {{47, 53, 84, 148, 258}, {67, 73, 102, 166, 258}, {85, 91, 120, 184, 258}, {103, 109, 138, 202, 266}},  // P = 8, W = 1..4
};

// ... and of topk_weighted_partial_kernel<W, KREG, P, TopkFilter> (profiles/search_filtered_topk.txt)
constexpr int FWTOPK_VGPRS[2][4][5] = {
    {{36, 48, 80, 142, 259}, {47, 58, 90, 152, 259}, {58, 69, 101, 163, 259}, {68, 79, 111, 173, 259}},     // P = 4, W = 1..4
    {{48, 56, 88, 150, 259}, {68, 74, 106, 168, 259}, {88, 94, 125, 187, 259}, {106, 112, 143, 205, 268}},  // P = 8, W = 1..4
};

int wtopk_seg_rows(int64_t Qn, int64_t G, int W, int k, int P, bool filtered) {
    return topk_seg_rows_table(Qn, G, (filtered ? FWTOPK_VGPRS : WTOPK_VGPRS)[P == 8][W - 1][topk_list_index(k)], (int64_t)1 << WKEY_SHIFT);
}

// the workspace of either weighted entry: its call does not name P, so room for the finer of the two segmentations
size_t wtopk_workspace(int64_t Qn, int64_t G, int W, int k, bool filtered) {
    if (W < 1 || W > 4) return 16;
    return topk_workspace_bytes(Qn, G, k,
                                [&] { return std::min(wtopk_seg_rows(Qn, G, W, k, 4, filtered), wtopk_seg_rows(Qn, G, W, k, 8, filtered)); });
}

// ---------------------------------------------------------------------------------------------------------------
// host: the "scans" of the one launch path (TopkCall, topk_run: hamming_shared.h).  A scan names one of the two kernels, holds its
// extra arguments and knows its key split, its segmentation, its workspace and the wording of its own refusals.
// ---------------------------------------------------------------------------------------------------------------
template <bool MASKED>
struct HammingScan {
    static constexpr int SHIFT = KEY_SHIFT;
    static constexpr const char *too_many_segments = "hamming_topk: gallery too large for one call (shard it)";
    TopkMask<MASKED> qm;
    int check(int W) const {   // the masked entry's own refusals
        if constexpr (MASKED) {
            CH_REQUIRE(qm.stride == 0 || qm.stride == W,
                       "hamming_topk_masked: mask_stride must be W (one mask per query) or 0 (one mask shared by all queries)");
            CH_REQUIRE(qm.mask != nullptr, "hamming_topk_masked: null q_mask");
        }
        return 0;
    }
    bool operands() const { return true; }   // the mask was checked above
    int seg_rows(int64_t Qn, int64_t G, int W, int k, bool filtered) const {
        return filtered ? ftopk_seg_rows(Qn, G, W, k, MASKED) : topk_seg_rows(Qn, G, k);
    }
    size_t workspace(int64_t Qn, int64_t G, int W, int k, bool filtered) const {
        return filtered ? ch_hamming_topk_filtered_workspace(Qn, G, W, k) : ch_hamming_topk_workspace(Qn, G, W, k);
    }
    template <int W, int KREG, class Filter>
    void launch(const TopkCall &c, const Filter &flt) const {
        hipLaunchKernelGGL((topk_partial_kernel<W, KREG, MASKED, Filter>), c.grid, dim3(256), 0, c.s, c.q, c.Qn, c.g, c.G, c.seg_rows, c.k,
                           c.part, qm, flt);
    }
};

template <int P>
struct WeightedScan {
    static constexpr int SHIFT = WKEY_SHIFT;
    static constexpr const char *too_many_segments =
        "hamming_topk_weighted: gallery too large for one call: more than 65,535 segments (shard it)";
    const uint64_t *planes;
    int check(int) const { return 0; }
    bool operands() const { return planes != nullptr; }
    int seg_rows(int64_t Qn, int64_t G, int W, int k, bool filtered) const { return wtopk_seg_rows(Qn, G, W, k, P, filtered); }
    size_t workspace(int64_t Qn, int64_t G, int W, int k, bool filtered) const { return wtopk_workspace(Qn, G, W, k, filtered); }
    template <int W, int KREG, class Filter>
    void launch(const TopkCall &c, const Filter &flt) const {
        hipLaunchKernelGGL((topk_weighted_partial_kernel<W, KREG, P, Filter>), c.grid, dim3(256), 0, c.s, c.q, planes, c.Qn, c.g, c.G,
                           c.seg_rows, c.k, c.part, flt);
    }
};

// the body of ch_hamming_topk_weighted and of its _filtered form: the check of P, then topk_run under that P's scan
template <class Filter>
int wtopk_run(const char *name, const uint64_t *q, const uint64_t *planes, int P, int64_t Qn, const uint64_t *g, int64_t G, int W, int k,
              int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *workspace, size_t workspace_bytes, void *stream,
              const Filter &flt) {
    CH_REQUIRE(P == 4 || P == 8, std::string(name) + ": P (weight bits) must be 4 or 8");
    if (P == 4)
        return topk_run(name, WeightedScan<4>{planes}, q, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace, workspace_bytes,
                        (hipStream_t)stream, flt);
    return topk_run(name, WeightedScan<8>{planes}, q, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace, workspace_bytes,
                    (hipStream_t)stream, flt);
}

}  // namespace

// ch_hamming_topk_workspace has never looked at W: 16 for non-positive Qn, G or k only
extern "C" size_t ch_hamming_topk_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k) {
    (void)W;
    return topk_workspace_bytes(Qn, G, k, [&] { return topk_seg_rows(Qn, G, k); });
}

extern "C" size_t ch_hamming_topk_weighted_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k) {
    return wtopk_workspace(Qn, G, W, k, false);
}

extern "C" int ch_hamming_topk(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t k,
                               int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *workspace,
                               size_t workspace_bytes, void *stream) {
    return topk_run("hamming_topk", HammingScan<false>{}, q, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace,
                    workspace_bytes, (hipStream_t)stream, TopkNoFilter{});
}

extern "C" int ch_hamming_topk_masked(const uint64_t *q, const uint64_t *q_mask, int32_t mask_stride, int64_t Qn, const uint64_t *g,
                                      int64_t G, int32_t W, int32_t k, int64_t g_index_base, int64_t *out_idx, int32_t *out_dist,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    return topk_run("hamming_topk_masked", HammingScan<true>{{q_mask, mask_stride}}, q, Qn, g, G, W, k, g_index_base, out_idx,
                    out_dist, workspace, workspace_bytes, (hipStream_t)stream, TopkNoFilter{});
}

extern "C" int ch_hamming_topk_weighted(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                                        int32_t W, int32_t k, int64_t g_index_base, int64_t *out_idx, int32_t *out_dist,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    return wtopk_run("hamming_topk_weighted", q, planes, P, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace, workspace_bytes,
                     stream, TopkNoFilter{});
}

// The filtered entries: their siblings' scans and checks with a TopkFilter.  Their segments follow the filtered instances' registers,
// so they have workspace functions of their own; the calls name neither the mask nor P: room for the finer of the two segmentations.
extern "C" size_t ch_hamming_topk_filtered_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k) {
    if (W < 1 || W > 4) return 16;
    return topk_workspace_bytes(Qn, G, k, [&] { return std::min(ftopk_seg_rows(Qn, G, W, k, false), ftopk_seg_rows(Qn, G, W, k, true)); });
}

extern "C" size_t ch_hamming_topk_weighted_filtered_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k) {
    return wtopk_workspace(Qn, G, W, k, true);
}

extern "C" int ch_hamming_topk_filtered(const uint64_t *q, const uint64_t *q_mask, int32_t mask_stride, int64_t Qn, const uint64_t *g,
                                        int64_t G, int32_t W, int32_t k, int64_t g_index_base, const uint64_t *allow, const int32_t *group,
                                        const int64_t *want, int32_t exclude, int64_t *out_idx, int32_t *out_dist, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    const TopkFilter flt{allow, group, want, g_index_base, (int)exclude};
    if (q_mask == nullptr)
        return topk_run("hamming_topk_filtered", HammingScan<false>{}, q, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace,
                        workspace_bytes, (hipStream_t)stream, flt);
    return topk_run("hamming_topk_filtered", HammingScan<true>{{q_mask, mask_stride}}, q, Qn, g, G, W, k, g_index_base, out_idx,
                    out_dist, workspace, workspace_bytes, (hipStream_t)stream, flt);
}

extern "C" int ch_hamming_topk_weighted_filtered(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g,
                                                 int64_t G, int32_t W, int32_t k, int64_t g_index_base, const uint64_t *allow,
                                                 const int32_t *group, const int64_t *want, int32_t exclude, int64_t *out_idx,
                                                 int32_t *out_dist, void *workspace, size_t workspace_bytes, void *stream) {
    return wtopk_run("hamming_topk_weighted_filtered", q, planes, P, Qn, g, G, W, k, g_index_base, out_idx, out_dist, workspace,
                     workspace_bytes, stream, TopkFilter{allow, group, want, g_index_base, (int)exclude});
}

extern "C" int ch_weight_planes(const float *codes, int64_t Qn, int32_t nbit, const uint64_t *mask, int32_t mask_stride, int32_t P,
                                uint64_t *out_planes, int32_t *out_wsum, void *stream) {
    CH_REQUIRE(P == 4 || P == 8, "weight_planes: P (weight bits) must be 4 or 8");
    CH_REQUIRE(nbit >= 1 && nbit <= 256, "weight_planes: nbit must be in [1, 256]");
    const int W = (nbit + 63) / 64;
    CH_REQUIRE(mask_stride == 0 || mask_stride == W,
               "weight_planes: mask_stride must be W (one mask per query) or 0 (one mask shared by all queries, or no mask)");
    CH_REQUIRE(Qn >= 0, "weight_planes: negative Qn");
    if (Qn == 0) return 0;
    CH_REQUIRE(codes && out_planes && out_wsum, "weight_planes: null pointer");
    const dim3 grid((unsigned)ceil_div64(Qn, 4));
    hipStream_t s = (hipStream_t)stream;
    if (P == 4)
        hipLaunchKernelGGL(weight_planes_kernel<4>, grid, dim3(256), 0, s, codes, Qn, (int)nbit, W, mask, (int)mask_stride, out_planes,
                           out_wsum);
    else
        hipLaunchKernelGGL(weight_planes_kernel<8>, grid, dim3(256), 0, s, codes, Qn, (int)nbit, W, mask, (int)mask_stride, out_planes,
                           out_wsum);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_hamming_subcode_dist(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, const int64_t *idx,
                                       int32_t k, int64_t g_index_base, int32_t nbit, int32_t nsub, int32_t *out, void *stream) {
    CH_REQUIRE(W >= 1 && W <= 4, "hamming_subcode_dist: 1 <= W <= 4 (nbit <= 256)");
    CH_REQUIRE(nbit >= 1 && nbit <= 64 * W, "hamming_subcode_dist: nbit must be in [1, 64 W]");
    CH_REQUIRE(nsub >= 1 && nbit % nsub == 0, "hamming_subcode_dist: nsub must divide nbit");
    CH_REQUIRE(k >= 1 && Qn >= 0 && G >= 0, "hamming_subcode_dist: bad sizes (k >= 1, Qn >= 0, G >= 0)");
    if (Qn == 0) return 0;
    CH_REQUIRE(q && idx && out && (g || G == 0), "hamming_subcode_dist: null pointer");
    hipStream_t s = (hipStream_t)stream;
    // the hits index the gallery, so they are checked HERE, on a host copy, before any kernel reads a row through them
    // (Qn * k indices: this is the tail of a search, not a scan)
    std::vector<int64_t> h((size_t)(Qn * k));
    CH_CHECK_HIP(hipMemcpyAsync(h.data(), idx, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, s));
    CH_CHECK_HIP(hipStreamSynchronize(s));
    for (int64_t v : h)
        CH_REQUIRE(v == -1 || (v >= g_index_base && v - g_index_base < G),
                   "hamming_subcode_dist: idx holds an index outside [g_index_base, g_index_base + G) that is not -1");
    hipLaunchKernelGGL(subcode_dist_kernel, dim3((unsigned)ceil_div64(Qn * k, 256)), dim3(256), 0, s, q, Qn, g, G, (int)W, idx, (int)k,
                       g_index_base, (int)(nbit / nsub), (int)nsub, out);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_topk_merge(const int64_t *idx_lists, const int32_t *dist_lists, int32_t nlists, int64_t Qn, int32_t k,
                             int64_t *out_idx, int32_t *out_dist, void *stream) {
    CH_REQUIRE(nlists >= 1 && k >= 1 && Qn >= 0, "topk_merge: bad sizes");
    if (Qn == 0) return 0;
    CH_REQUIRE(idx_lists && dist_lists && out_idx && out_dist, "topk_merge: null pointer");
    hipLaunchKernelGGL(topk_merge_lists_kernel, dim3((unsigned)ceil_div64(Qn, 4)), dim3(256), 0, (hipStream_t)stream, idx_lists,
                       dist_lists, nlists, Qn, k, out_idx, out_dist);
    CH_LAUNCH_CHECK();
    return 0;
}
