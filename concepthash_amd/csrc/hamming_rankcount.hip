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
#include <algorithm>
#include <string>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "hamming_shared.h"

namespace {

constexpr int RC_BLK = 256;          // lanes of a workgroup of the two scans
constexpr int RC_MAX_LIST = 8192;    // longest list held in LDS: 8 B per key + 4 B per bin = 96 KB
constexpr int RC_TQ = 16;            // queries per workgroup of the collect pass
constexpr int RC_QUEUE = 8192;       // ... and the (query, row) pairs its LDS queue holds: two trips' worth at the most (32 KB)
constexpr int RC_ROW_BITS = 27;      // a queue entry = query in tile << 27 | row in segment: segments of at most 2^27 rows
static_assert(RC_QUEUE >= 2 * RC_BLK * RC_TQ && RC_TQ <= (1 << (32 - RC_ROW_BITS)), "queue entry layout");

// ---------------------------------------------------------------------------------------------------------------
// collect: the keys of the relevant rows
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

__device__ __forceinline__ bool masks_meet(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, int LW) {
    bool r = false;
    for (int w = 0; w < LW; ++w) r |= (a[w] & b[w]) != 0ull;
    return r;
}

// One workgroup per (tile of RC_TQ queries, gallery segment); lanes stride over the segment's rows, and a row's label is loaded once for
// the whole tile (the queries of a tile are walked by a workgroup-uniform loop: their labels arrive through the scalar data path).
// WRITE = false (the entry's offsets == NULL): count[q] += relevant rows.  WRITE = true: count[q] is the fill of the query's slice
// keys[offsets[q] .. offsets[q + 1]): every relevant row reserves a slot with an atomic add and leaves its key there (any order inside
// a slice).  A slot past the slice is never written.
template <bool WRITE>
__global__ __launch_bounds__(RC_BLK) void rank_collect_kernel(const uint64_t *__restrict__ q, const uint64_t *__restrict__ planes, int P,
                                                              int64_t Qn, const uint64_t *__restrict__ g, int64_t G, int W,
                                                              const void *q_labels, const void *g_labels, int LW, int seg_rows,
                                                              int64_t g_index_base, const int64_t *__restrict__ offsets,
                                                              uint32_t *__restrict__ count, uint64_t *__restrict__ keys) {
    const int64_t q0 = (int64_t)blockIdx.x * RC_TQ;
    const int nq = (int)min((int64_t)RC_TQ, Qn - q0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t g0 = (int64_t)blockIdx.y * seg_rows;
    const int n = (int)min((int64_t)seg_rows, G - g0);
    const int32_t *gl32 = (const int32_t *)g_labels, *ql32 = (const int32_t *)q_labels;
    const uint64_t *glm = (const uint64_t *)g_labels, *qlm = (const uint64_t *)q_labels;
    if constexpr (!WRITE) {
        int32_t qlab[RC_TQ];
        uint32_t mine[RC_TQ];
#pragma unroll
        for (int t = 0; t < RC_TQ; ++t) {
            qlab[t] = (LW == 0 && t < nq) ? ql32[q0 + t] : 0;
            mine[t] = 0u;
        }
        for (int r = tid; r < n; r += RC_BLK) {
            const int64_t j = g0 + r;
            const int32_t glab = LW == 0 ? gl32[j] : 0;
#pragma unroll
            for (int t = 0; t < RC_TQ; ++t) {
                bool rel = false;
                if (t < nq) rel = LW == 0 ? glab == qlab[t] : masks_meet(qlm + (q0 + t) * LW, glm + j * LW, LW);
                mine[t] += rel ? 1u : 0u;
            }
        }
#pragma unroll
        for (int t = 0; t < RC_TQ; ++t) {
            uint32_t c = mine[t];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0 && c != 0u && t < nq) atomicAdd(count + q0 + t, c);
        }
    } else {
        // Relevant (query, row) pairs are rare and scattered over the lanes, and a key costs a slot reservation (an atomic that returns) and
        // a distance: done where the pair is found, one or two lanes of a wave would pay that latency pair after pair.  Instead a lane that
        // finds a pair leaves (query in tile, row in segment) in an LDS queue, and the workgroup empties the queue with every lane busy --
        // whenever the next trip might not fit (a trip adds at most RC_BLK * RC_TQ pairs), and at the end.
        __shared__ uint32_t queue[RC_QUEUE];
        __shared__ uint32_t queued;
        if (tid == 0) queued = 0u;
        __syncthreads();
        auto drain = [&](uint32_t cnt) {   // called by the whole workgroup with the count every lane read between two barriers
            for (uint32_t e = tid; e < cnt; e += RC_BLK) {
                const uint32_t entry = queue[e];
                const int64_t qi = q0 + (entry >> RC_ROW_BITS), j = g0 + (entry & ((1u << RC_ROW_BITS) - 1u));
                const int64_t off = offsets[qi];
                const uint32_t room = (uint32_t)(offsets[qi + 1] - off);
                const uint32_t slot = atomicAdd(count + qi, 1u);
                if (slot < room)
                    keys[off + slot] = ((uint64_t)weighted_dist_row(q + qi * W, planes + qi * P * W, P, W, g + j * W) << 32) |
                                       (uint64_t)(g_index_base + j);
            }
            __syncthreads();
            if (tid == 0) queued = 0u;
            __syncthreads();
        };
        for (int r0 = 0; r0 < n; r0 += RC_BLK) {   // the same trips for every lane: the barriers below are a workgroup's
            const int r = r0 + tid;
            if (r < n) {
                const int64_t j = g0 + r;
                const int32_t glab = LW == 0 ? gl32[j] : 0;
                for (int t = 0; t < nq; ++t) {
                    const int64_t qi = q0 + t;
                    if (LW == 0 ? glab == ql32[qi] : masks_meet(qlm + qi * LW, glm + j * LW, LW))
                        queue[atomicAdd(&queued, 1u)] = ((uint32_t)t << RC_ROW_BITS) | (uint32_t)r;
                }
            }
            __syncthreads();
            const uint32_t cnt = queued;   // the same value in every lane: nobody adds to the queue before the next barrier
            if (cnt > (uint32_t)(RC_QUEUE - RC_BLK * RC_TQ))
                drain(cnt);
            else
                __syncthreads();
        }
        drain(queued);
    }
}

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

// #{j < n : list[j] < key}
__device__ __forceinline__ uint32_t keys_below(const uint64_t *list, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (list[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The rows [0, nrows) of a segment against one query, two rows per lane and trip (both rows' loads are out before the first distance).
// list / bins: the query's sorted keys and its bins, in LDS or in global memory.  A key above `last` = list[n - 1] is done after the
// compare; any other has keys_below <= n - 1, so bins[n] does not exist.
template <int W, int P>
__device__ __forceinline__ void rank_count_rows(const uint32_t (&qs)[2 * W], const uint32_t (&ps)[P][2 * W],
                                                const uint64_t *__restrict__ gp, int nrows, uint64_t row0, const uint64_t *list,
                                                uint32_t n, uint64_t last, uint32_t *bins) {
    for (int r = threadIdx.x; r < nrows; r += 2 * RC_BLK) {
        const bool two = r + RC_BLK < nrows;
        const int r1 = two ? r + RC_BLK : r;
        uint64_t ga[W], gb[W];
#pragma unroll
        for (int w = 0; w < W; ++w) ga[w] = gp[(size_t)r * W + w];
#pragma unroll
        for (int w = 0; w < W; ++w) gb[w] = gp[(size_t)r1 * W + w];
        const uint64_t ka = ((uint64_t)weighted_dist_uniform<W, P>(qs, ps, ga) << 32) | (row0 + (uint64_t)r);
        const uint64_t kb1 = ((uint64_t)weighted_dist_uniform<W, P>(qs, ps, gb) << 32) | (row0 + (uint64_t)r1);
        const uint64_t kb = two ? kb1 : ~0ull;   // no second row: above every key
        if (ka <= last) atomicAdd(bins + keys_below(list, n, ka), 1u);
        if (kb <= last) atomicAdd(bins + keys_below(list, n, kb), 1u);
    }
}

// One workgroup per (query, gallery segment).  A query without a relevant row ends at its first branch.  A list of at most list_cap
// keys lives in LDS with its bins, which leave through global atomic adds at the end (segments add up); a longer one is searched where
// it lies, in global memory, and its bins are added to directly.
template <int W, int P>
__global__ __launch_bounds__(RC_BLK) void rank_count_kernel(const uint64_t *__restrict__ q, const uint64_t *__restrict__ planes,
                                                            const uint64_t *__restrict__ g, int64_t G, int seg_rows,
                                                            int64_t g_index_base, const int64_t *__restrict__ offsets,
                                                            const uint64_t *__restrict__ keys, int list_cap,
                                                            uint32_t *__restrict__ bins) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];   // [list_cap] keys, then [list_cap] uint32 bins
    const int64_t qi = blockIdx.x;
    const int64_t off = offsets[qi];
    const int64_t n64 = offsets[qi + 1] - off;
    if (n64 <= 0) return;   // workgroup-uniform
    const uint32_t n = (uint32_t)n64;
    const int tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.y * seg_rows;
    const int nrows = (int)min((int64_t)seg_rows, G - g0);
    uint32_t qs[2 * W], ps[P][2 * W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t v = q[qi * W + w];
        qs[2 * w] = __builtin_amdgcn_readfirstlane((uint32_t)v);
        qs[2 * w + 1] = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t v = planes[(qi * P + p) * W + w];
            ps[p][2 * w] = __builtin_amdgcn_readfirstlane((uint32_t)v);
            ps[p][2 * w + 1] = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        }
    }
    const uint64_t *list = keys + off;
    const uint64_t last = list[n - 1];
    const uint64_t *gp = g + g0 * W;
    const uint64_t row0 = (uint64_t)(g_index_base + g0);
    if (n <= (uint32_t)list_cap) {
        uint32_t *lds_bins = (uint32_t *)(lds_keys + list_cap);
        for (uint32_t i = tid; i < n; i += RC_BLK) {
            lds_keys[i] = list[i];
            lds_bins[i] = 0u;
        }
        __syncthreads();
        rank_count_rows<W, P>(qs, ps, gp, nrows, row0, lds_keys, n, last, lds_bins);
        __syncthreads();
        for (uint32_t i = tid; i < n; i += RC_BLK) {
            const uint32_t c = lds_bins[i];
            if (c != 0u) atomicAdd(bins + off + i, c);
        }
    } else {
        rank_count_rows<W, P>(qs, ps, gp, nrows, row0, list, n, last, bins + off);
    }
}

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

// f(std::integral_constant<int, P>) for P in {4, 8}
template <class F>
int dispatch_p(int P, F &&f) {
    if (P == 4) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 8>{});
}

// what the collect and count entries check alike
int check_scan_sizes(const char *who, int P, int64_t Qn, int64_t G, int W, int64_t g_index_base) {
    const std::string at = std::string(who) + ": ";
    CH_REQUIRE(P == 4 || P == 8, at + "P (weight bits) must be 4 or 8");
    CH_REQUIRE(W >= 1 && W <= 4, at + "1 <= W <= 4 (nbit <= 256)");
    CH_REQUIRE(Qn >= 0 && G >= 0, at + "negative sizes");
    CH_REQUIRE(Qn <= 0x7FFFFFFFll, at + "one workgroup column per query (Qn < 2^31)");
    CH_REQUIRE(g_index_base >= 0 && g_index_base + G <= 0x100000000ll, at + "keys hold 32-bit global indices (g_index_base + G <= 2^32)");
    return 0;
}

}  // namespace

extern "C" int ch_hamming_rank_collect(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                                       int32_t W, const void *q_labels, const void *g_labels, int32_t LW, int64_t g_index_base,
                                       const int64_t *offsets, uint32_t *count, uint64_t *keys, void *stream) {
    if (int e = check_scan_sizes("hamming_rank_collect", P, Qn, G, W, g_index_base)) return e;
    CH_REQUIRE(LW >= 0, "hamming_rank_collect: negative LW");
    if (Qn == 0 || G == 0) return 0;
    CH_REQUIRE(g && q_labels && g_labels && count, "hamming_rank_collect: null pointer");
    CH_REQUIRE(offsets == nullptr || (q && planes && keys), "hamming_rank_collect: null pointer (q, planes and keys go with offsets)");
    // segments so that a small query set still fills the chip; a workgroup walks at least 1,024 labels
    const int64_t tiles = ceil_div64(Qn, RC_TQ);
    const int64_t nseg = std::max<int64_t>(ceil_div64(G, (int64_t)1 << RC_ROW_BITS),
                                           std::min<int64_t>(std::min<int64_t>(65535, ceil_div64(G, 1024)), ceil_div64(4096, tiles)));
    const int64_t rows = ceil_div64(G, nseg);   // at most 2^27: a queue entry of the write pass holds the row in its segment
    const dim3 grid((unsigned)tiles, (unsigned)ceil_div64(G, rows));
    if (offsets == nullptr)
        hipLaunchKernelGGL(rank_collect_kernel<false>, grid, dim3(RC_BLK), 0, (hipStream_t)stream, q, planes, (int)P, Qn, g, G, (int)W,
                           q_labels, g_labels, (int)LW, (int)rows, g_index_base, offsets, count, keys);
    else
        hipLaunchKernelGGL(rank_collect_kernel<true>, grid, dim3(RC_BLK), 0, (hipStream_t)stream, q, planes, (int)P, Qn, g, G, (int)W,
                           q_labels, g_labels, (int)LW, (int)rows, g_index_base, offsets, count, keys);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_hamming_rank_count(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                                     int32_t W, int64_t g_index_base, int32_t seg_rows, const int64_t *offsets, const uint64_t *keys,
                                     int32_t list_cap, uint32_t *bins, void *stream) {
    if (int e = check_scan_sizes("hamming_rank_count", P, Qn, G, W, g_index_base)) return e;
    CH_REQUIRE(seg_rows >= 1, "hamming_rank_count: seg_rows must be >= 1");
    CH_REQUIRE(list_cap >= 1 && list_cap <= RC_MAX_LIST, "hamming_rank_count: list_cap must be in [1, 8192]");
    if (Qn == 0 || G == 0) return 0;
    CH_REQUIRE(q && planes && g && offsets && keys && bins, "hamming_rank_count: null pointer");
    CH_REQUIRE(ceil_div64(G, seg_rows) <= 65535, "hamming_rank_count: too many gallery segments (raise seg_rows)");
    const dim3 grid((unsigned)Qn, (unsigned)ceil_div64(G, seg_rows));
    const size_t lds = (size_t)list_cap * (sizeof(uint64_t) + sizeof(uint32_t));
    return dispatch_w(W, [&](auto w) {
        return dispatch_p(P, [&](auto p) {
            constexpr int Wc = decltype(w)::value, Pc = decltype(p)::value;
            static ch_once_per_device lds_once;   // one per instance of this body, i.e. per kernel
            if (int e = ch_func_max_lds((const void *)rank_count_kernel<Wc, Pc>, RC_MAX_LIST * 12, lds_once)) return e;
            hipLaunchKernelGGL((rank_count_kernel<Wc, Pc>), grid, dim3(RC_BLK), lds, (hipStream_t)stream, q, planes, g, G, (int)seg_rows,
                               g_index_base, offsets, keys, (int)list_cap, bins);
            CH_LAUNCH_CHECK();
            return 0;
        });
    });
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
