// What the top-k scan (hamming_topk.hip), the mAP passes (hamming.hip) and the rank pass (hamming_rank.hip) share: the chained popcount,
// the query load and the plain Hamming distance built on them; for the latter two, which keep a tile's per-distance counters in LDS, the
// shape of a workgroup and the W -> instance dispatch.  Everything here has internal linkage.
#pragma once
#include <cstdint>
#include <type_traits>

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

}  // namespace
