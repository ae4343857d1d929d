// Evaluation of the weighted (asymmetric) ranking on packed codes (gfx950): mAP@R, P@k and R@k by RANK COUNTING.
//
// The ranking is ascending key(g) = D(q, g) << 32 | global index of g, with D the weighted distance of hamming_topk.hip,
// D = sum_p 2^p popcount((q ^ g) & planes[q, p]).  D reaches 65,280, so the mAP passes of hamming.hip, which
// keep one LDS counter per (query, distance), cannot serve it.  Only the ranks of a query's RELEVANT rows enter its AP, so:
//     collect     the keys of every query's relevant rows, into its slice of a CSR buffer (the caller sorts every slice);
//     rank count  with r_0 < r_1 < ... < r_{n-1} the sorted slice, every gallery row adds one to bins[#{j : r_j < key(row)}].  Then
//                 rank(r_j) = sum_{b <= j} bins[b] (1-based) and its rank among the relevant rows is j + 1.  A row whose key exceeds
//                 r_{n-1} would land in bin n, which nobody reads: one compare and it is done -- with trained codes nearly every row;
//     AP          one lane per query walks its bins: prefix, remove_first, the fixed-point AP terms under up to 16 rank limits.
// bins are integer sums over gallery rows: gallery segments (blockIdx.y) add up in any order and give the same bits.
// Nothing of size Qn x G is written.
// The collect and the count kernel, their launches and the bodies of their entries are templates on the ranking (hamming_shared.h);
// this file holds what the weighted ranking supplies to them -- its distance in two forms, its operands and their checks -- and the AP
// pass.  hamming_ternary.hip and dense_rank.hip supply the same under the ternary and the dense distances.
#include <algorithm>
#include <string>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "hamming_shared.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// collect: the keys of the relevant rows (rank_collect_kernel, hamming_shared.h, under the distance below)
// ---------------------------------------------------------------------------------------------------------------
// D of one (query, row) pair with everything read from memory: the collect pass pays it for relevant rows only (G / C of G).
__device__ __forceinline__ uint32_t weighted_dist_row(const uint64_t *__restrict__ q, const uint64_t *__restrict__ pl, int P, int W,
                                                      const uint64_t *__restrict__ g) {
    uint32_t d = 0;
    for (int w = 0; w < W; ++w) {
        const uint64_t x = q[w] ^ g[w];
        for (int p = 0; p < P; ++p) d += (uint32_t)__builtin_popcountll(x & pl[p * W + w]) << p;
    }
    return d;
}

struct WeightedRow {
    const uint64_t *q, *planes;
    int P;
    __device__ __forceinline__ uint32_t row(int64_t qi, int W, const uint64_t *__restrict__ g, int64_t j) const {
        return weighted_dist_row(q + qi * W, planes + qi * P * W, P, W, g + j * W);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// rank count: the Qn x G scan
// ---------------------------------------------------------------------------------------------------------------
// D with the query's code and plane words WAVE-UNIFORM and the gallery row the lane's own.  A VOP3 instruction of this target takes one
// SGPR operand, so (q ^ g) & plane cannot name q and the plane word as two SGPRs of one v_bitop3_b32.  Written as x = q ^ g, x & plane,
// the compiler keeps the q words in SGPRs and copies the plane words to VGPRs once, in front of the row loop (2 P W registers): one
// v_bitop3_b32 (SGPR q, VGPR plane, VGPR g) and one chained v_bcnt per word and plane -- 2 P instructions per word, as in the top-k
// scan -- then its Horner chain.
template <int W, int P>
__device__ __forceinline__ uint32_t weighted_dist_uniform(const uint32_t (&qs)[2 * W], const uint32_t (&ps)[P][2 * W],
                                                          const uint64_t (&g)[W]) {
    uint32_t acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t x0 = qs[2 * w] ^ (uint32_t)g[w], x1 = qs[2 * w + 1] ^ (uint32_t)(g[w] >> 32);
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = bcnt_acc(x0 & ps[p][2 * w], acc[p]);
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = bcnt_acc(x1 & ps[p][2 * w + 1], acc[p]);
    }
    return horner2(acc);
}

// what rank_count_kernel (hamming_shared.h) takes as its distance: the query's words and planes, read once into wave-uniform registers
template <int W, int P>
struct WeightedUniform {
    static constexpr int ROW = W;
    struct Regs {
        uint32_t qs[2 * W], ps[P][2 * W];
        const uint64_t *gp;   // the segment's first row
    };
    const uint64_t *q, *planes;
    __device__ __forceinline__ void load(Regs &r, int64_t qi, const uint64_t *__restrict__ g, int64_t g0) const {
        r.gp = g + g0 * ROW;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t v = q[qi * W + w];
            r.qs[2 * w] = __builtin_amdgcn_readfirstlane((uint32_t)v);
            r.qs[2 * w + 1] = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint64_t v = planes[(qi * P + p) * W + w];
                r.ps[p][2 * w] = __builtin_amdgcn_readfirstlane((uint32_t)v);
                r.ps[p][2 * w + 1] = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
            }
        }
    }
    __device__ __forceinline__ static uint32_t at(const Regs &r, const uint64_t (&g)[W]) { return weighted_dist_uniform<W, P>(r.qs, r.ps, g); }
    __device__ __forceinline__ void rows(const Regs &r, int nrows, uint64_t row0, const uint64_t *list, uint32_t n, uint64_t last,
                                         uint32_t *bins) const {
        rank_count_rows<WeightedUniform>(r, r.gp, nrows, row0, list, n, last, bins);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// AP from the bins
// ---------------------------------------------------------------------------------------------------------------
// One lane per query: rank(r_j) is the running sum of its bins.  remove_first (the semantics of ap_account, hamming.hip): the dropped
// rank-1 row is relevant iff rank(r_0) == 1 (frel); a relevant row at rank 1 is skipped, every other row counts with rank - 1 and
// relrank - frel.  Ranks ascend along the list, so the walk ends at the first rank past the largest limit.  lims is padded to
// MAX_LIMITS with its last entry (fill_limits): all 16 accumulate, the first nlim are written.
__global__ __launch_bounds__(256) void rank_ap_kernel(int64_t Qn, const int64_t *__restrict__ offsets, const uint32_t *__restrict__ bins,
                                                      RankLimits lims, int nlim, int remove_first, unsigned long long *__restrict__ out_S,
                                                      uint32_t *__restrict__ out_nrel, int32_t *__restrict__ out_total) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (qi >= Qn) return;
    const int64_t off = offsets[qi];
    const uint32_t n = (uint32_t)(offsets[qi + 1] - off);
    unsigned long long S[MAX_LIMITS];
    uint32_t nrel[MAX_LIMITS];
#pragma unroll
    for (int r = 0; r < MAX_LIMITS; ++r) {
        S[r] = 0ull;
        nrel[r] = 0u;
    }
    uint32_t rank = 0, frel = 0;
    for (uint32_t j = 0; j < n; ++j) {
        rank += bins[off + j];
        uint32_t rk = rank, relrank = j + 1u;
        if (remove_first) {
            if (j == 0u) frel = rank == 1u ? 1u : 0u;
            if (rk == 1u) continue;
            rk -= 1u;
            relrank -= frel;
        }
        if (rk > lims.lim[MAX_LIMITS - 1]) break;
        const unsigned long long term = fixdiv32(relrank, rk);
#pragma unroll
        for (int r = 0; r < MAX_LIMITS; ++r) {
            const bool in = rk <= lims.lim[r];
            S[r] += in ? term : 0ull;
            nrel[r] += in ? 1u : 0u;
        }
    }
#pragma unroll
    for (int r = 0; r < MAX_LIMITS; ++r) {
        if (r < nlim) {
            out_S[(size_t)r * Qn + qi] = S[r];
            out_nrel[(size_t)r * Qn + qi] = nrel[r];
        }
    }
    if (out_total != nullptr) out_total[qi] = (int32_t)(n - (remove_first ? frel : 0u));
}

// what rank_collect_run / rank_count_run (hamming_shared.h) take as the ranking
struct WeightedRanking {
    static constexpr const char *with_offsets = "q, planes and keys";
    const uint64_t *q, *planes;
    int P, W;
    int check(const char *who, int64_t Qn, int64_t G, int64_t g_index_base) const {
        CH_REQUIRE(P == 4 || P == 8, std::string(who) + ": P (weight bits) must be 4 or 8");
        return check_rank_sizes(who, Qn, G, W, g_index_base);
    }
    bool operands() const { return q && planes; }
    template <class F> int collect(F &&f) const { return f(WeightedRow{q, planes, P}, W); }
    template <class F>
    int count(F &&f) const {
        return dispatch_w(W, [&](auto w) {
            constexpr int Wc = decltype(w)::value;
            return P == 4 ? f(WeightedUniform<Wc, 4>{q, planes}) : f(WeightedUniform<Wc, 8>{q, planes});
        });
    }
};

}  // namespace

extern "C" int ch_hamming_rank_collect(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                                       int32_t W, const void *q_labels, const void *g_labels, int32_t LW, int64_t g_index_base,
                                       const int64_t *offsets, uint32_t *count, uint64_t *keys, void *stream) {
    return rank_collect_run("hamming_rank_collect", WeightedRanking{q, planes, (int)P, (int)W}, Qn, g, G, q_labels, g_labels, (int)LW,
                            g_index_base, offsets, count, keys, (hipStream_t)stream);
}

extern "C" int ch_hamming_rank_count(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                                     int32_t W, int64_t g_index_base, int32_t seg_rows, const int64_t *offsets, const uint64_t *keys,
                                     int32_t list_cap, uint32_t *bins, void *stream) {
    return rank_count_run("hamming_rank_count", WeightedRanking{q, planes, (int)P, (int)W}, Qn, g, G, g_index_base, (int)seg_rows, offsets,
                          keys, (int)list_cap, bins, (hipStream_t)stream);
}

extern "C" int ch_hamming_rank_ap(int64_t Qn, const int64_t *offsets, const uint32_t *bins, const int64_t *rank_limits, int32_t nlimits,
                                  int32_t remove_first, unsigned long long *out_S, uint32_t *out_nrel, int32_t *out_total,
                                  void *stream) {
    CH_REQUIRE_NLIMITS("hamming_rank_ap");
    CH_REQUIRE(Qn >= 0, "hamming_rank_ap: negative Qn");
    if (Qn == 0) return 0;
    CH_REQUIRE(offsets && out_S && out_nrel, "hamming_rank_ap: null pointer");   // bins may be NULL when every list is empty
    RankLimits lims;
    if (int e = fill_limits("hamming_rank_ap", rank_limits, nlimits, lims)) return e;
    hipLaunchKernelGGL(rank_ap_kernel, dim3((unsigned)ceil_div64(Qn, 256)), dim3(256), 0, (hipStream_t)stream, Qn, offsets, bins, lims,
                       (int)nlimits, (int)remove_first, out_S, out_nrel, out_total);
    CH_LAUNCH_CHECK();
    return 0;
}
