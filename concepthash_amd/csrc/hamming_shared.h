// What the top-k scans of hamming.hip (plain and masked Hamming distance) and hamming_weighted.hip (weighted distance) share: the
// chained popcount, the query load, the merge of per-segment key lists and the segment sizing.  Everything here has internal linkage.
#pragma once
#include <algorithm>
#include <cstdint>

#include "ch_common.h"

namespace {

// The scan is VALU-issue bound, so its inner loop is written down to the instruction:
// v_bcnt_u32_b32 d, x, acc = popcount(x) + acc: chaining the accumulate operand keeps a distance at 2 instructions per 32-bit
// word (left to itself the compiler re-associates into separate counts + v_add3: one more instruction per row);
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t d;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
    return d;
}

template <int W>
__device__ __forceinline__ void load_query(uint32_t (&q)[2 * W], const uint64_t *qp, int64_t qi, int64_t Qn) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t v = qi < Qn ? qp[qi * W + w] : 0ull;
        q[2 * w] = (uint32_t)v;
        q[2 * w + 1] = (uint32_t)(v >> 32);
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

// Gallery rows per segment of a top-k scan whose kernel keeps `per_cu` workgroups of four waves resident per CU and whose keys hold
// `max_rows` rows per segment.
// (tile, segment) workgroups for ONE full round and never a few more: ceil(2048 / tiles) segments put 2,134 workgroups on the 2,048
// slots at the NABirds size (97 tiles): a second round for 86 of them doubled the launch (0.38 -> 0.2 ms).  Segments not shorter than
// 256 rows.
inline int topk_seg_rows_for(int64_t Qn, int64_t G, int per_cu, int64_t max_rows) {
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

}  // namespace
