// What the top-k scans (hamming_topk.hip, hamming_ternary.hip), the mAP passes (hamming.hip), the rank pass (hamming_rank.hip) and the
// rank-counting evaluations (hamming_rankcount.hip: weighted; hamming_ternary.hip: ternary) share: the chained popcount, the query load
// and the plain Hamming distance built on them; for the mAP and rank passes, which keep a tile's per-distance counters in LDS, the
// shape of a workgroup and the W -> instance dispatch; the Horner chain of the weighted distance; the fixed-point quotient and the
// rank limits of an AP pass; the top-k scan with the distance and the filter as template arguments, the merge of its segment
// lists, the list-length table, the residency rule, the workspace formula and the launch path, and the collect and count passes of rank counting, each with the distance as a template argument.  Everything here has internal linkage.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>

#include "ch_common.h"

namespace {

// The scans are VALU-issue bound, so their inner loops are written down to the instruction:
// v_bcnt_u32_b32 d, x, acc = popcount(x) + acc: chaining the accumulate operand keeps a distance at 2 instructions per 32-bit
// word (left to itself the compiler re-associates into separate counts + v_add3: one more instruction per row);
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t d;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
    return d;
}

// the W words of query qi as 2 W registers; a lane past Qn holds zeros
template <int W>
__device__ __forceinline__ void load_query(uint32_t (&q)[2 * W], const uint64_t *qp, int64_t qi, int64_t Qn) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t v = qi < Qn ? qp[qi * W + w] : 0ull;
        q[2 * w] = (uint32_t)v;
        q[2 * w + 1] = (uint32_t)(v >> 32);
    }
}

template <int W>
__device__ __forceinline__ int hamming(const uint32_t (&q)[2 * W], const uint64_t *__restrict__ g) {
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t gw = g[w];
        d = bcnt_acc(q[2 * w] ^ (uint32_t)gw, d);
        d = bcnt_acc(q[2 * w + 1] ^ (uint32_t)(gw >> 32), d);
    }
    return (int)d;
}

// A scan with counters in LDS, [buckets][lanes] x 4 B, one lane per query: lanes per workgroup and distance buckets of W-word codes
constexpr int scan_lanes(int W) { return W <= 2 ? 256 : 128; }
constexpr int scan_buckets(int W) { return 64 * W + 1; }

// f(std::integral_constant<int, W>) for a W the caller has checked to be in [1, 4]
template <class F>
int dispatch_w(int W, F &&f) {
    switch (W) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// sum_p 2^p a[p] as a Horner chain of P - 1 v_lshl_add_u32, in one asm block.  Written as d = (d << 1) + a[p] the chain is
// redistributed into a sum of shifted terms a little further each time the code around it is inlined one level up, and what gets
// selected from that follows the number of levels: 8 instructions for 8 planes while the scan was written out in each kernel, 9 to
// 10 behind topk_scan and its distance callable.  One block, not one asm per step: between two dependent asm statements that end
// up next to each other the compiler puts an s_nop.
__device__ __forceinline__ uint32_t horner2(const uint32_t (&a)[4]) {
    uint32_t d;
    asm("v_lshl_add_u32 %0, %4, 1, %3\n\t"
        "v_lshl_add_u32 %0, %0, 1, %2\n\t"
        "v_lshl_add_u32 %0, %0, 1, %1"
        : "=&v"(d)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]));
    return d;
}
__device__ __forceinline__ uint32_t horner2(const uint32_t (&a)[8]) {
    uint32_t d;
    asm("v_lshl_add_u32 %0, %8, 1, %7\n\t"
        "v_lshl_add_u32 %0, %0, 1, %6\n\t"
        "v_lshl_add_u32 %0, %0, 1, %5\n\t"
        "v_lshl_add_u32 %0, %0, 1, %4\n\t"
        "v_lshl_add_u32 %0, %0, 1, %3\n\t"
        "v_lshl_add_u32 %0, %0, 1, %2\n\t"
        "v_lshl_add_u32 %0, %0, 1, %1"
        : "=&v"(d)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]));
    return d;
}

// floor(a * 2^32 / b) for 1 <= a <= b < 2^32, exact: double estimate (hardware reciprocal + one Newton step, relative error
// ~2^-51, i.e. < 2^-18 absolute on a quotient <= 2^32) + integer correction.  No IEEE division sequence.
__device__ __forceinline__ unsigned long long fixdiv32(uint32_t a, uint32_t b) {
    const unsigned long long num = (unsigned long long)a << 32;
    const double bd = (double)b;
    double r = __builtin_amdgcn_rcp(bd);
    r = __builtin_fma(r, __builtin_fma(-bd, r, 1.0), r);
    unsigned long long qq = (unsigned long long)((double)a * 4294967296.0 * r);
    long long rem = (long long)(num - qq * (unsigned long long)b);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (rem < 0) {
            qq -= 1;
            rem += b;
        }
        if (rem >= (long long)b) {
            qq += 1;
            rem -= b;
        }
    }
    return qq;
}

constexpr int MAX_LIMITS = 16;
struct RankLimits {
    uint32_t lim[MAX_LIMITS];  // mAP@R cut-offs of one AP pass; 0xFFFFFFFF = the whole ranking
};

// The two checks of an entry that takes rank limits (`who`: its name in the messages): their number, in front of the entry's other
// checks, and -- behind them -- their order, which fills lims.
#define CH_REQUIRE_NLIMITS(who) CH_REQUIRE(nlimits >= 1 && nlimits <= MAX_LIMITS && rank_limits != nullptr, who ": 1 <= nlimits <= 16")
int fill_limits(const char *who, const int64_t *rank_limits, int nlimits, RankLimits &lims) {
    for (int i = 0; i < MAX_LIMITS; ++i) {
        const int64_t r = rank_limits[i < nlimits ? i : nlimits - 1];
        lims.lim[i] = (r <= 0 || r >= 0xFFFFFFFFll) ? 0xFFFFFFFFu : (uint32_t)r;
        CH_REQUIRE(i == 0 || lims.lim[i] >= lims.lim[i - 1], std::string(who) + ": rank limits must ascend (<= 0 = unlimited, last)");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The top-k scan (hamming_topk.hip: plain, masked, weighted; hamming_ternary.hip: ternary): per (query tile, gallery segment)
// partial lists, their merge, the segment sizing and the one launch path of every entry.
// ---------------------------------------------------------------------------------------------------------------
// key = dist << SHIFT | row with the (wave-uniform) row number taken from an SGPR: one v_lshl_or_b32 (the compiler's own form is a
// shift plus v_or3 with the row's low bits as a literal).
template <int SHIFT>
__device__ __forceinline__ uint32_t make_key(uint32_t d, uint32_t row_uniform) {
    uint32_t key;
    asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(key) : "v"(d), "n"(SHIFT), "s"(row_uniform));
    return key;
}

// The filter of a scan (ch_*_topk_filtered; DESIGN.md section 2.0, "filtered search"): which gallery rows may be hits at all.  Row r of
// THIS call's gallery is admitted for query i iff
//     allow == NULL or bit r & 63 of allow[r >> 6] is set                               (one bitmap for all queries), and
//     want == NULL or want[i] < 0 or (grp(r) == want[i]) != exclude                     (per query),
// grp(r) = group[r] (int32 >= 0) or, where group == NULL, base + r: a row is its own group.  A row that is not admitted for a lane gets
// the empty-slot key 0xFFFFFFFF, which is above every real key of every scan (asserted beside KEY_SHIFT / WKEY_SHIFT in hamming_topk.hip
// and beside TKEY_SHIFT in hamming_ternary.hip), so the insertion network and the merge see nothing new.  The filter is a template
// argument from the entry to the kernel (topk_run, topk_launch, a scan's launch, the one __global__ template of each distance, which
// takes it by value): the unfiltered scans carry TopkNoFilter, an empty argument as TopkMask<false> is, and none of the filter's code.
struct TopkNoFilter {
    static constexpr bool ON = false;
};
struct TopkFilter {
    static constexpr bool ON = true;
    const uint64_t *allow;   // [ceil(G / 64)] or NULL
    const int32_t *group;    // [G] or NULL
    const int64_t *want;     // [Qn] or NULL
    int64_t base;            // g_index_base: the group of row r where group == NULL
    int exclude;             // 0: only the wanted group, 1: every group but it
};

// Segment blockIdx.y of the gallery against query qi (a lane past Qn scans too -- its registers hold zeros -- and stores nothing):
// from the empty list to the store of its k smallest keys.  W: the 64-bit words of a gallery ROW (a two-plane row has twice the words
// of a code); dist: const uint64_t * (those words) -> uint32_t.  UB (4 or 2): the rows of one block of scalar loads -- two buffers of
// UB * W * 2 SGPRs have to fit beside everything else that is wave-uniform.
// Under a TopkFilter both of its parts are run-time, wave-uniform conditions of ONE instance.  The allow-list lives on the scalar path:
// the gallery walk is wave-uniform, so the word of the bitmap that holds a block's rows is an SGPR pair, loaded once per 64 rows (a
// segment starts anywhere, so a block may straddle two words: the second one is loaded then and stays for the rows behind), and a block
// whose UB bits are all zero is left by a wave-uniform branch in front of its distances, keys and threshold test.  The group part costs
// one compare and one select per row: the row's group id (or its number in the segment) is wave-uniform, the lane holds its query's
// wanted id as 32 bits (-2, which no row has, where the query wants nothing or an id that no row of this segment can have).
template <int W, int KREG, int SHIFT, int UB = 4, class Dist, class Filter = TopkNoFilter>
__device__ __forceinline__ void topk_scan(const Dist &dist, int64_t qi, int64_t Qn, const uint64_t *__restrict__ g, int64_t G,
                                          int seg_rows, int k, uint32_t *__restrict__ part, const Filter &flt = Filter{}) {
    static_assert(UB == 4 || UB == 2, "rows per block");
    constexpr bool FILTERED = Filter::ON;
    const int seg = blockIdx.y;
    const int64_t g0 = (int64_t)seg * seg_rows;
    const int n = (int)min((int64_t)seg_rows, G - g0);
    uint32_t list[KREG];
#pragma unroll
    for (int i = 0; i < KREG; ++i) list[i] = 0xFFFFFFFFu;
    const uint64_t *gp = g + g0 * W;
    auto insert = [&](uint32_t key) {
        if (__builtin_amdgcn_ballot_w64(key < list[KREG - 1]) != 0ull) {
#pragma unroll
            for (int i = 0; i < KREG; ++i) {
                const uint32_t lo = min(list[i], key);
                key = max(list[i], key);
                list[i] = lo;
            }
        }
    };
    // the filter's registers: per lane the wanted id and whether there is one; wave-uniform the bitmap word in hand and its number
    [[maybe_unused]] int32_t wv = -2;
    [[maybe_unused]] bool has = false;
    [[maybe_unused]] bool grouped = false, own_row = false;
    [[maybe_unused]] uint64_t aword = 0ull;
    [[maybe_unused]] int aword_at = -1;              // ... counted from the word of the segment's first row, so 32 bits do
    [[maybe_unused]] const uint64_t *ap = nullptr;   // that word
    [[maybe_unused]] int a0 = 0;                     // the segment's first row in it
    if constexpr (FILTERED) {
        if (flt.allow != nullptr) ap = flt.allow + (g0 >> 6);
        a0 = (int)(g0 & 63);
        grouped = flt.want != nullptr;
        own_row = grouped && flt.group == nullptr && flt.exclude != 0;   // "every row but the query's own"
        if (grouped && qi < Qn) {
            const int64_t w = flt.want[qi];
            // group == NULL: the one row base + r == w, as its number in this segment; a group plane: ids are int32 >= 0
            const int64_t v = flt.group != nullptr ? w : w - flt.base - g0;
            has = w >= 0;
            wv = (has && v >= 0 && v <= 0x7FFFFFFFll) ? (int32_t)v : -2;
        }
    }
    // bits [0, cnt) = the allow bits of rows [row, row + cnt) of the segment (cnt <= UB; all of them < n)
    [[maybe_unused]] auto allow_bits = [&](int row, int cnt) -> uint32_t {
        const uint32_t all = (1u << cnt) - 1u;
        if constexpr (FILTERED) {
            if (ap == nullptr) return all;
            const int r = a0 + row;
            const int w = r >> 6;
            const int b = r & 63;
            if (w != aword_at) {
                aword = ap[w];
                aword_at = w;
            }
            uint64_t bits = aword >> b;
            if (b + cnt > 64) {   // the block's last rows are in the next word (it exists: they are rows of the gallery)
                aword = ap[w + 1];
                aword_at = w + 1;
                bits |= aword << (64 - b);
            }
            return (uint32_t)bits & all;
        } else {
            return all;
        }
    };
    // a lane's key of a row under the group part: the empty slot where the row's group is not admitted for its query
    [[maybe_unused]] auto group_key = [&](uint32_t key, int32_t grp) -> uint32_t {
        if constexpr (FILTERED) {
            const bool hit = grp == wv;
            const bool rej = flt.exclude != 0 ? hit : (has && !hit);
            return rej ? 0xFFFFFFFFu : key;
        } else {
            return key;
        }
    };
    // UB gallery rows per trip: one wide scalar load (the next block is requested before this one is consumed), UB keys, ONE
    // threshold test on their minimum; the insertion network runs only if some lane beats its list.
    uint64_t bufA[UB * W], bufB[UB * W];
    [[maybe_unused]] int32_t grpA[UB], grpB[UB];   // FILTERED: the rows' group ids (or their numbers in the segment) beside their words
    auto load_block = [&](uint64_t (&dst)[UB * W], [[maybe_unused]] int32_t (&grp)[UB], int row) {
#pragma unroll
        for (int t = 0; t < UB * W; ++t) dst[t] = gp[(size_t)row * W + t];
        if constexpr (FILTERED) {
            if (grouped) {
#pragma unroll
                for (int u = 0; u < UB; ++u) grp[u] = flt.group != nullptr ? flt.group[g0 + row + u] : row + u;
            }
        }
    };
    auto scan_block = [&](const uint64_t (&blk)[UB * W], [[maybe_unused]] const int32_t (&grp)[UB], int row) {
        [[maybe_unused]] uint32_t bits = 0u;
        if constexpr (FILTERED) {
            bits = allow_bits(row, UB);
            if (bits == 0u) return;   // wave-uniform: no row of the block is admitted for anybody
        }
        uint32_t key[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) key[u] = make_key<SHIFT>(dist(blk + u * W), (uint32_t)(row + u));
        if constexpr (FILTERED) {
            if (grouped) {
                // own_row: a lane's one row is in one block of one segment -- one test per block says whether any lane's is in this one
                bool any = true;
                if (own_row) any = __builtin_amdgcn_ballot_w64((uint32_t)(wv - row) < (uint32_t)UB) != 0ull;
                if (any) {
#pragma unroll
                    for (int u = 0; u < UB; ++u) key[u] = group_key(key[u], grp[u]);
                }
            }
            if (bits != (1u << UB) - 1u) {
#pragma unroll
                for (int u = 0; u < UB; ++u) key[u] = ((bits >> u) & 1u) != 0u ? key[u] : 0xFFFFFFFFu;
            }
        }
        uint32_t kmin;
        if constexpr (UB == 4)
            kmin = min(min(key[0], key[1]), min(key[2], key[3]));
        else
            kmin = min(key[0], key[1]);
        if (__builtin_amdgcn_ballot_w64(kmin < list[KREG - 1]) != 0ull) {
#pragma unroll
            for (int u = 0; u < UB; ++u) insert(key[u]);
        }
    };
    // two blocks per iteration with the two SGPR buffers taking turns: no register copies between trips
    int j = 0;
    if (n >= UB) load_block(bufA, grpA, 0);
    for (; j + 2 * UB <= n; j += 2 * UB) {
        load_block(bufB, grpB, j + UB);
        scan_block(bufA, grpA, j);
        if (j + 3 * UB <= n) load_block(bufA, grpA, j + 2 * UB);
        scan_block(bufB, grpB, j + UB);
    }
    if (j + UB <= n) {  // an odd number of whole blocks: the last one is already in bufA
        scan_block(bufA, grpA, j);
        j += UB;
    }
    if constexpr (FILTERED) {
        for (; j < n; ++j) {   // the tail filters row by row
            if (allow_bits(j, 1) == 0u) continue;
            uint32_t key = (dist(gp + (size_t)j * W) << SHIFT) | (uint32_t)j;
            if (grouped) key = group_key(key, flt.group != nullptr ? flt.group[g0 + j] : j);
            insert(key);
        }
    } else {
        for (; j < n; ++j) insert((dist(gp + (size_t)j * W) << SHIFT) | (uint32_t)j);
    }
    if (qi < Qn) {
        uint32_t *o = part + ((size_t)seg * Qn + qi) * k;
#pragma unroll
        for (int i = 0; i < KREG; ++i)
            if (i < k) o[i] = list[i];
    }
}

// The merge of per-segment key lists, key = dist << SHIFT | row-in-segment (0xFFFFFFFF = empty slot).
// one wave per query: repeatedly extract the smallest composite (dist, global row) above the previous one
template <int SHIFT>
__global__ __launch_bounds__(256) void topk_merge_keys_kernel(const uint32_t *__restrict__ part, int nseg, int64_t Qn, int k,
                                                              int seg_rows, int64_t g_index_base, int64_t *out_idx,
                                                              int32_t *out_dist) {
    constexpr uint32_t MASK = (1u << SHIFT) - 1;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (qi >= Qn) return;
    const int ncand = nseg * k;
    unsigned long long prev = 0ull;  // composite + 1 of the last output (0 = none yet)
    for (int r = 0; r < k; ++r) {
        unsigned long long best = ~0ull;
        for (int c = lane; c < ncand; c += 64) {
            const int s = c / k, i = c - s * k;
            const uint32_t key = part[((size_t)s * Qn + qi) * k + i];
            if (key == 0xFFFFFFFFu) continue;
            const unsigned long long comp =
                ((unsigned long long)(key >> SHIFT) << 40) | ((unsigned long long)s * seg_rows + (key & MASK));
            if (comp + 1 > prev && comp < best) best = comp;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        if (lane == 0) {
            if (best == ~0ull) {
                out_idx[qi * k + r] = -1;
                out_dist[qi * k + r] = -1;
            } else {
                out_idx[qi * k + r] = g_index_base + (int64_t)(best & ((1ull << 40) - 1));
                out_dist[qi * k + r] = (int32_t)(best >> 40);
            }
        }
        if (best == ~0ull) {
            // nothing left: fill the rest
            for (int rr = r + 1; rr < k; ++rr)
                if (lane == 0) {
                    out_idx[qi * k + rr] = -1;
                    out_dist[qi * k + rr] = -1;
                }
            return;
        }
        prev = best + 1;
    }
}

// Gallery rows per segment of a scan whose kernel keeps `per_cu` workgroups of four waves resident per CU and whose keys hold
// `max_rows` rows per segment.
// (tile, segment) workgroups for ONE full round and never a few more: ceil(2048 / tiles) segments put 2,134 workgroups on the 2,048
// slots at the NABirds size (97 tiles): a second round for 86 of them doubled the launch (0.38 -> 0.2 ms).  Segments not shorter than
// 256 rows.
int topk_seg_rows_for(int64_t Qn, int64_t G, int per_cu, int64_t max_rows) {
    const int64_t slots = 256 * per_cu;
    const int64_t tiles = ceil_div64(Qn, 256);
    int64_t nseg = std::max<int64_t>(1, slots / tiles);
    // ... and not more segments than needed: every segment starts with empty lists, so its first ~640 rows run the insertion
    // network for some lane of the wave almost every row, and the merge cost grows with the segment count -- segments of >= 4,096
    // rows as long as two workgroups per CU remain (NABirds size: 6 segments instead of 21, 0.45 -> 0.37 ms; the 1M-row scan keeps 32)
    nseg = std::min(nseg, std::max<int64_t>(std::max<int64_t>(1, ceil_div64(512, tiles)), G / 4096));
    int64_t rows = ceil_div64(G, nseg);
    if (rows < 256) rows = 256;
    if (rows > max_rows) rows = max_rows;
    return (int)rows;
}

// THE residency rule: workgroups of four waves that a CU keeps of a scan kernel with `vgprs` registers (the scans have no LDS):
// min(8, 512 / VGPRs rounded up to the allocation unit of 8).
int topk_per_cu(int vgprs) { return std::max(1, std::min(8, 512 / std::max(8, (vgprs + 7) / 8 * 8))); }

// ... and the table form of a segment rule: the segments of a kernel from its VGPR count in the family's table of code-object metadata
int topk_seg_rows_table(int64_t Qn, int64_t G, int vgprs, int64_t max_rows) {
    return topk_seg_rows_for(Qn, G, topk_per_cu(vgprs), max_rows);
}

// The list lengths: a scan keeps KREG = 10 / 16 / 32 / 64 / 128 keys per lane, the shortest list that holds k.  k <= 10
// (PRs = [1, 5, 10]): exactly k entries, so the insertion threshold is the k-th key.  topk_list_index: the position of k's list, which
// is also the last index of every VGPR table.
constexpr int TOPK_KREG[5] = {10, 16, 32, 64, 128};
int topk_list_index(int k) {
    int i = 0;
    while (i < 4 && k > TOPK_KREG[i]) ++i;
    return i;
}

// The workspace of a call: one list of k keys per (segment, query), and 16 bytes where the sizes have no segmentation.  rows: () -> the
// rows of a segment, asked for sizes that have one only.
template <class Rows>
size_t topk_workspace_bytes(int64_t Qn, int64_t G, int k, const Rows &rows) {
    if (Qn <= 0 || G <= 0 || k <= 0) return 16;
    return (size_t)(ceil_div64(G, rows()) * Qn * k) * sizeof(uint32_t) + 16;
}

// host: one launch path.  A "scan" names one kernel family, holds its extra arguments and knows its key split, its segmentation, its
// workspace and the wording of its own refusals; topk_run is the body of every top-k entry point.  The filter (TopkNoFilter or
// TopkFilter) is a typed argument from the entry to the kernel: seg_rows() and workspace() take Filter::ON, launch() the filter.
struct TopkCall {   // what every partial launch takes
    const uint64_t *q;
    int64_t Qn;
    const uint64_t *g;
    int64_t G;
    int seg_rows, k;
    uint32_t *part;
    dim3 grid;
    hipStream_t s;
};

template <int W, class Scan, class Filter>
void topk_launch_k(const Scan &scan, const TopkCall &c, const Filter &flt) {
    switch (topk_list_index(c.k)) {
        case 0: return scan.template launch<W, TOPK_KREG[0]>(c, flt);
        case 1: return scan.template launch<W, TOPK_KREG[1]>(c, flt);
        case 2: return scan.template launch<W, TOPK_KREG[2]>(c, flt);
        case 3: return scan.template launch<W, TOPK_KREG[3]>(c, flt);
        default: return scan.template launch<W, TOPK_KREG[4]>(c, flt);
    }
}

template <class Scan, class Filter>
void topk_launch(const Scan &scan, int W, const TopkCall &c, const Filter &flt) {
    switch (W) {
        case 1: return topk_launch_k<1>(scan, c, flt);
        case 2: return topk_launch_k<2>(scan, c, flt);
        case 3: return topk_launch_k<3>(scan, c, flt);
        default: return topk_launch_k<4>(scan, c, flt);
    }
}

// The body of ch_hamming_topk / _masked / _weighted and ch_ternary_topk and of their _filtered forms: the checks in the order the
// entries have always made them (`name` opens the messages), partial lists, merge.  A segment's rows must fit under the key's distance:
// the scan's seg_rows() answers at most 2^SHIFT, checked here in front of the launch.  flt: TopkNoFilter{}, or the TopkFilter of a
// _filtered entry (its base is the call's g_index_base).
template <class Scan, class Filter>
int topk_run(const char *name, const Scan &scan, const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int W,
             int k, int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *workspace, size_t workspace_bytes, hipStream_t s,
             const Filter &flt) {
    const std::string at = std::string(name) + ": ";
    CH_REQUIRE(W >= 1 && W <= 4, at + "1 <= W <= 4 (nbit <= 256)");
    CH_REQUIRE(k >= 1 && k <= 128, at + "1 <= k <= 128");
    CH_REQUIRE(Qn >= 0 && G >= 0, at + "negative sizes");
    if constexpr (Filter::ON) CH_REQUIRE(flt.exclude == 0 || flt.exclude == 1, at + "exclude must be 0 or 1");
    if (int e = scan.check(W)) return e;
    if (Qn == 0) return 0;
    CH_REQUIRE(q && scan.operands() && out_idx && out_dist, at + "null pointer");
    if (G == 0) {
        CH_CHECK_HIP(hipMemsetAsync(out_idx, 0xFF, sizeof(int64_t) * Qn * k, s));
        CH_CHECK_HIP(hipMemsetAsync(out_dist, 0xFF, sizeof(int32_t) * Qn * k, s));
        return 0;
    }
    CH_REQUIRE(g != nullptr, at + "null gallery");
    const int seg_rows = scan.seg_rows(Qn, G, W, k, Filter::ON);
    CH_REQUIRE(seg_rows >= 1 && (int64_t)seg_rows <= ((int64_t)1 << Scan::SHIFT), at + "segment longer than the key's row field");
    const int64_t nseg = ceil_div64(G, seg_rows);
    CH_REQUIRE(nseg <= 65535, Scan::too_many_segments);
    CH_REQUIRE(workspace && workspace_bytes >= scan.workspace(Qn, G, W, k, Filter::ON), at + "workspace too small");
    uint32_t *part = (uint32_t *)workspace;
    topk_launch(scan, W, TopkCall{q, Qn, g, G, seg_rows, k, part, dim3((unsigned)ceil_div64(Qn, 256), (unsigned)nseg), s}, flt);
    CH_LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_merge_keys_kernel<Scan::SHIFT>, dim3((unsigned)ceil_div64(Qn, 4)), dim3(256), 0, s, part, (int)nseg, Qn, k,
                       seg_rows, g_index_base, out_idx, out_dist);
    CH_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Evaluation by rank counting: the collect and the count pass -- kernels, launches and the body of their entries -- once, with the
// ranking a template argument (hamming_rankcount.hip: the weighted distance; hamming_ternary.hip: the ternary one; dense_rank.hip: the
// three dense ones).  The ranking is ascending key(g) = dist(q, g) << 32 | global index of g.
// ---------------------------------------------------------------------------------------------------------------
constexpr int RC_BLK = 256;          // lanes of a workgroup of the two scans
constexpr int RC_MAX_LIST = 8192;    // longest list held in LDS: 8 B per key + 4 B per bin = 96 KB
constexpr int RC_TQ = 16;            // queries per workgroup of the collect pass
constexpr int RC_QUEUE = 8192;       // ... and the (query, row) pairs its LDS queue holds: two trips' worth at the most (32 KB)
constexpr int RC_ROW_BITS = 27;      // a queue entry = query in tile << 27 | row in segment: segments of at most 2^27 rows
static_assert(RC_QUEUE >= 2 * RC_BLK * RC_TQ && RC_TQ <= (1 << (32 - RC_ROW_BITS)), "queue entry layout");

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
// RowDist: the distance of one (query, row) pair with everything read from memory -- the collect pass pays it for relevant rows only
// (G / C of G): dist.row(qi, W, g, j) -> uint32_t, g the gallery's first word.
template <bool WRITE, class RowDist>
__global__ __launch_bounds__(RC_BLK) void rank_collect_kernel(RowDist dist, int64_t Qn, const uint64_t *__restrict__ g, int64_t G, int W,
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
                if (slot < room) keys[off + slot] = ((uint64_t)dist.row(qi, W, g, j) << 32) | (uint64_t)(g_index_base + j);
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
// UniDist: a bit-plane distance with the query's words WAVE-UNIFORM (UniDist::Regs, filled by its load()) and the gallery row -- ROW
// 64-bit words -- the lane's own: UniDist::at(regs, row words) -> uint32_t.  Its rows() (below) is one call of this on regs.gp.
template <class UniDist>
__device__ __forceinline__ void rank_count_rows(const typename UniDist::Regs &regs, const uint64_t *__restrict__ gp, int nrows,
                                                uint64_t row0, const uint64_t *list, uint32_t n, uint64_t last, uint32_t *bins) {
    constexpr int ROW = UniDist::ROW;
    for (int r = threadIdx.x; r < nrows; r += 2 * RC_BLK) {
        const bool two = r + RC_BLK < nrows;
        const int r1 = two ? r + RC_BLK : r;
        uint64_t ga[ROW], gb[ROW];
#pragma unroll
        for (int w = 0; w < ROW; ++w) ga[w] = gp[(size_t)r * ROW + w];
#pragma unroll
        for (int w = 0; w < ROW; ++w) gb[w] = gp[(size_t)r1 * ROW + w];
        const uint64_t ka = ((uint64_t)UniDist::at(regs, ga) << 32) | (row0 + (uint64_t)r);
        const uint64_t kb1 = ((uint64_t)UniDist::at(regs, gb) << 32) | (row0 + (uint64_t)r1);
        const uint64_t kb = two ? kb1 : ~0ull;   // no second row: above every key
        if (ka <= last) atomicAdd(bins + keys_below(list, n, ka), 1u);
        if (kb <= last) atomicAdd(bins + keys_below(list, n, kb), 1u);
    }
}

// One workgroup per (query, gallery segment).  A query without a relevant row ends at its first branch.  A list of at most list_cap
// keys lives in LDS with its bins, which leave through global atomic adds at the end (segments add up); a longer one is searched where
// it lies, in global memory, and its bins are added to directly.
// Count: what a ranking brings to this shell -- the workgroup's registers (Count::Regs, filled by load(regs, qi, g, g0): the query and
// where the segment's rows begin) and the row loop rows(regs, nrows, row0, list, n, last, bins): rank_count_rows for the bit-plane
// distances, its own for the dense ones.
template <class Count>
__global__ __launch_bounds__(RC_BLK) void rank_count_kernel(Count dist, const uint64_t *__restrict__ g, int64_t G, int seg_rows,
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
    typename Count::Regs regs;
    dist.load(regs, qi, g, g0);
    const uint64_t *list = keys + off;
    const uint64_t last = list[n - 1];
    const uint64_t row0 = (uint64_t)(g_index_base + g0);
    if (n <= (uint32_t)list_cap) {
        uint32_t *lds_bins = (uint32_t *)(lds_keys + list_cap);
        for (uint32_t i = tid; i < n; i += RC_BLK) {
            lds_keys[i] = list[i];
            lds_bins[i] = 0u;
        }
        __syncthreads();
        dist.rows(regs, nrows, row0, lds_keys, n, last, lds_bins);
        __syncthreads();
        for (uint32_t i = tid; i < n; i += RC_BLK) {
            const uint32_t c = lds_bins[i];
            if (c != 0u) atomicAdd(bins + off + i, c);
        }
    } else {
        dist.rows(regs, nrows, row0, list, n, last, bins + off);
    }
}

// what the collect and count entries of every ranking check alike, next to the checks of their own operands
int check_rank_sizes(const char *who, int64_t Qn, int64_t G, int W, int64_t g_index_base) {
    const std::string at = std::string(who) + ": ";
    CH_REQUIRE(W >= 1 && W <= 4, at + "1 <= W <= 4 (nbit <= 256)");
    CH_REQUIRE(Qn >= 0 && G >= 0, at + "negative sizes");
    CH_REQUIRE(Qn <= 0x7FFFFFFFll, at + "one workgroup column per query (Qn < 2^31)");
    CH_REQUIRE(g_index_base >= 0 && g_index_base + G <= 0x100000000ll, at + "keys hold 32-bit global indices (g_index_base + G <= 2^32)");
    return 0;
}

// the launch of a collect pass on checked arguments: segments so that a small query set fills the chip, of at least 1,024 labels
template <class RowDist>
int rank_collect_launch(const RowDist &dist, int64_t Qn, const uint64_t *g, int64_t G, int W, const void *q_labels, const void *g_labels,
                        int LW, int64_t g_index_base, const int64_t *offsets, uint32_t *count, uint64_t *keys, hipStream_t s) {
    const int64_t tiles = ceil_div64(Qn, RC_TQ);
    const int64_t nseg = std::max<int64_t>(ceil_div64(G, (int64_t)1 << RC_ROW_BITS),
                                           std::min<int64_t>(std::min<int64_t>(65535, ceil_div64(G, 1024)), ceil_div64(4096, tiles)));
    const int64_t rows = ceil_div64(G, nseg);   // at most 2^27: a queue entry of the write pass holds the row in its segment
    const dim3 grid((unsigned)tiles, (unsigned)ceil_div64(G, rows));
    const auto kernel = offsets == nullptr ? rank_collect_kernel<false, RowDist> : rank_collect_kernel<true, RowDist>;
    hipLaunchKernelGGL(kernel, grid, dim3(RC_BLK), 0, s, dist, Qn, g, G, W, q_labels, g_labels, LW, (int)rows, g_index_base, offsets, count,
                       keys);
    CH_LAUNCH_CHECK();
    return 0;
}

// ... and of a count pass
template <class Count>
int rank_count_launch(const Count &dist, int64_t Qn, const uint64_t *g, int64_t G, int64_t g_index_base, int seg_rows,
                      const int64_t *offsets, const uint64_t *keys, int list_cap, uint32_t *bins, hipStream_t s) {
    const dim3 grid((unsigned)Qn, (unsigned)ceil_div64(G, seg_rows));
    const size_t lds = (size_t)list_cap * (sizeof(uint64_t) + sizeof(uint32_t));
    static ch_once_per_device lds_once;   // one per instance of this body, i.e. per kernel
    if (int e = ch_func_max_lds((const void *)rank_count_kernel<Count>, RC_MAX_LIST * 12, lds_once)) return e;
    hipLaunchKernelGGL((rank_count_kernel<Count>), grid, dim3(RC_BLK), lds, s, dist, g, G, seg_rows, g_index_base, offsets, keys, list_cap,
                       bins);
    CH_LAUNCH_CHECK();
    return 0;
}

// The bodies of the ch_*_rank_collect and ch_*_rank_count entries, in the manner of topk_run: the checks in the order the entries have
// always made them (`who` opens the messages), then the launch.  A ranking holds its operands: check() makes its own checks and
// check_rank_sizes in its own order, operands() says whether the query side is there (with_offsets names it in a refusal), and
// collect(f) / count(f) call f(RowDist, W) / f(Count) under the instance that its sizes select.
template <class Ranking>
int rank_collect_run(const char *who, const Ranking &rk, int64_t Qn, const uint64_t *g, int64_t G, const void *q_labels,
                     const void *g_labels, int LW, int64_t g_index_base, const int64_t *offsets, uint32_t *count, uint64_t *keys,
                     hipStream_t s) {
    const std::string at = std::string(who) + ": ";
    if (int e = rk.check(who, Qn, G, g_index_base)) return e;
    CH_REQUIRE(LW >= 0, at + "negative LW");
    if (Qn == 0 || G == 0) return 0;
    CH_REQUIRE(g && q_labels && g_labels && count, at + "null pointer");
    CH_REQUIRE(offsets == nullptr || (rk.operands() && keys), at + "null pointer (" + Ranking::with_offsets + " go with offsets)");
    return rk.collect([&](const auto &dist, int W) {
        return rank_collect_launch(dist, Qn, g, G, W, q_labels, g_labels, LW, g_index_base, offsets, count, keys, s);
    });
}

template <class Ranking>
int rank_count_run(const char *who, const Ranking &rk, int64_t Qn, const uint64_t *g, int64_t G, int64_t g_index_base, int seg_rows,
                   const int64_t *offsets, const uint64_t *keys, int list_cap, uint32_t *bins, hipStream_t s) {
    const std::string at = std::string(who) + ": ";
    if (int e = rk.check(who, Qn, G, g_index_base)) return e;
    CH_REQUIRE(seg_rows >= 1, at + "seg_rows must be >= 1");
    CH_REQUIRE(list_cap >= 1 && list_cap <= RC_MAX_LIST, at + "list_cap must be in [1, 8192]");
    if (Qn == 0 || G == 0) return 0;
    CH_REQUIRE(rk.operands() && g && offsets && keys && bins, at + "null pointer");
    CH_REQUIRE(ceil_div64(G, seg_rows) <= 65535, at + "too many gallery segments (raise seg_rows)");
    return rk.count([&](const auto &dist) { return rank_count_launch(dist, Qn, g, G, g_index_base, seg_rows, offsets, keys, list_cap, bins, s); });
}

}  // namespace
