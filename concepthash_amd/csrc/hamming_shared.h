// What the top-k scan (hamming_topk.hip), the mAP passes (hamming.hip), the rank pass (hamming_rank.hip) and the evaluation of the
// weighted ranking (hamming_rankcount.hip) share: the chained popcount, the query load and the plain Hamming distance built on them;
// for the mAP and rank passes, which keep a tile's per-distance counters in LDS, the shape of a workgroup and the W -> instance
// dispatch; the Horner chain of the weighted distance; the fixed-point quotient and the rank limits of an AP pass.  Everything here
// has internal linkage.
#pragma once
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

}  // namespace
