// Tie expectation: the MEAN of AP@R, hits@k and R@k over every order of the gallery rows that share a Hamming distance, each bucket
// independently and uniformly permuted ("tie expectation"; the tie bracket of hamming.hip gives the two extremes
// of the same set of orders).  Input: the whole-gallery bucket counts, as for the bracket.  One wave per query, four per workgroup.
//
// Arithmetic: fp64 throughout, and every operation rounds once, in the order written here: this file is compiled with
// -ffp-contract=off (concepthash_amd/build.py) and without any fast-math flag, so there is no fused multiply-add the source does not
// spell (it spells none), `/` is the correctly rounded IEEE division, and nothing is re-associated.  The error bound of
// tests/tie_expected_ref.py (`error_bound`) counts exactly these roundings.
//
// With B rows and K relevant rows ranked before a stretch of m consecutive ranks B+1 .. B+m on which h relevant rows lie uniformly,
//   T(B, K, m, h) = (h / m) [ (K + 1) L + ((h - 1) / (m - 1)) M ],   L = sum_{i=1..m} 1 / (B + i),   M = sum_{i=1..m} (i - 1) / (B + i)
// is the expected sum of their precision terms.  M is m - (B + 1) L: it is summed as written, all terms positive, so the cancellation
// of the subtracted form (an absolute error of (B + 1) times that of L) never arises.
#include "hamming_shared.h"

namespace {

constexpr int MAX_KS = 16;
struct RankKs {
    uint32_t k[MAX_KS];   // the depths of hits@k / R@k; lane t of a wave owns k[t]
};

struct ExpectedOut {
    double *ap, *hits, *recall;
};

// Butterfly sum: every step adds two partial sums, and a + b == b + a, so the association order is fixed by the lane numbers alone
// and all 64 lanes end with the same bits.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_incl_prod_f64(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        if (lane >= o) v *= t;
    }
    return v;
}
__device__ __forceinline__ uint32_t limit_of(const RankLimits &lims, int l) {   // wave-uniform l: a chain of scalar selects
    uint32_t v = lims.lim[0];
#pragma unroll
    for (int i = 1; i < MAX_LIMITS; ++i) v = (l == i) ? lims.lim[i] : v;
    return v;
}

// L(B, m) and M(B, m): lane j takes the terms i = j + 1, j + 65, ... in ascending order, then the butterfly.  Every term is positive.
__device__ __forceinline__ void rank_sums(uint64_t B, uint32_t m, int lane, double &L, double &M) {
    double aL = 0.0, aM = 0.0;
    for (uint64_t i0 = 0; i0 < (uint64_t)m; i0 += 64u) {
        const uint64_t i = i0 + (uint64_t)lane;   // the term of rank B + i + 1
        if (i < (uint64_t)m) {
            const double inv = 1.0 / (double)(B + i + 1u);
            aL += inv;
            aM += (double)i * inv;
        }
    }
    L = wave_sum_f64(aL);
    M = wave_sum_f64(aM);
}

// The bucket (n rows, r relevant) that a limit cuts after `take` of its rows, 0 < take < n: the number h of relevant rows among the
// ranked ones is hypergeometric, and E = sum_h P(h) (S + T(B, K, take, h)) / (K + h).  The weights come from the ratio recurrence
// P(h + 1) / P(h) = (r - h)(take - h) / ((h + 1)(n - r - take + h + 1)), outward from the mode in both directions with the mode's
// weight set to 1, and are normalised by their sum; 64 consecutive h per trip, the running product by a wave scan.  The pmf is
// log-concave: past the mode the ratio rho is below 1 and falls, so after a weight w the remaining mass is at most w rho / (1 - rho).  A
// direction ends at the end of the feasible range, or at the end of a trip once that bound is under 2^-70 (of the mode's weight, hence
// of the sum).  Work: O(kept terms) -- a few standard deviations of h, never take^2.
__device__ double cut_expectation(uint64_t B, uint64_t K, double S, uint32_t n, uint32_t r, uint32_t take, int lane) {
    const uint32_t irr = n - r;
    const uint32_t tmin = take > irr ? take - irr : 0u, tmax = min(r, take);
    double L, M;
    rank_sums(B, take, lane, L, M);
    const double A = (double)(K + 1u) * L;
    const double C = take > 1u ? M / (double)(take - 1u) : 0.0;
    auto value = [&](uint64_t h) -> double {   // (S + T(B, K, take, h)) / (K + h); 0 without a relevant row
        if (K + h == 0u) return 0.0;
        const double T = h ? ((double)h / (double)take) * (A + (double)(h - 1u) * C) : 0.0;
        return (S + T) / (double)(K + h);
    };
    const double md = floor(((double)take + 1.0) * ((double)r + 1.0) / ((double)n + 2.0));
    const uint32_t mode = md >= (double)tmax ? tmax : (md <= (double)tmin ? tmin : (uint32_t)md);
    const double cut = 0x1p-70;
    double num = 0.0, den = 0.0;
    // upwards, the mode included: lane j of trip c holds h = mode + 64 c + j
    double carry = 1.0;
    for (uint64_t h0 = mode;; h0 += 64u) {
        const uint64_t h = h0 + (uint64_t)lane;
        const bool on = h <= (uint64_t)tmax;
        double f = 0.0;   // P(h) / P(h - 1); 1 at the mode; 0 past the range, which zeroes every later weight
        if (on)
            f = h == (uint64_t)mode ? 1.0
                                    : ((double)((uint64_t)r - h + 1u) * (double)((uint64_t)take - h + 1u)) /
                                          ((double)h * (double)((uint64_t)irr + h - (uint64_t)take));
        const double w = carry * wave_incl_prod_f64(f, lane);
        if (on) {
            num += w * value(h);
            den += w;
        }
        carry = __shfl(w, 63, 64);
        const uint64_t hl = h0 + 63u;
        bool stop = hl >= (uint64_t)tmax;
        if (!stop) {
            const double rho = ((double)((uint64_t)r - hl) * (double)((uint64_t)take - hl)) /
                               ((double)(hl + 1u) * (double)((uint64_t)irr + hl + 1u - (uint64_t)take));
            stop = rho < 1.0 && carry * rho < cut * (1.0 - rho);
        }
        if (__builtin_amdgcn_readfirstlane((int)stop)) break;
    }
    // downwards: lane j of trip c holds h = mode - 1 - 64 c - j
    if (mode > tmin) {
        const uint64_t span = (uint64_t)(mode - tmin);   // h = mode - off for off = 1 .. span
        carry = 1.0;
        for (uint64_t c = 0;; c += 64u) {
            const uint64_t off = c + (uint64_t)lane + 1u;
            const bool on = off <= span;
            const uint64_t h = on ? (uint64_t)mode - off : (uint64_t)tmin;
            double f = 0.0;   // P(h) / P(h + 1)
            if (on)
                f = ((double)(h + 1u) * (double)((uint64_t)irr + h + 1u - (uint64_t)take)) /
                    ((double)((uint64_t)r - h) * (double)((uint64_t)take - h));
            const double w = carry * wave_incl_prod_f64(f, lane);
            if (on) {
                num += w * value(h);
                den += w;
            }
            carry = __shfl(w, 63, 64);
            const uint64_t offl = c + 64u;
            bool stop = offl >= span;
            if (!stop) {
                const uint64_t hl = (uint64_t)mode - offl;   // > tmin
                const double rho = ((double)hl * (double)((uint64_t)irr + hl - (uint64_t)take)) /
                                   ((double)((uint64_t)r - hl + 1u) * (double)((uint64_t)take - hl + 1u));
                stop = rho < 1.0 && carry * rho < cut * (1.0 - rho);
            }
            if (__builtin_amdgcn_readfirstlane((int)stop)) break;
        }
    }
    return wave_sum_f64(num) / wave_sum_f64(den);   // den >= 1: the mode's weight
}

// One walk over a query's buckets, ascending distance; (dn, dr) rows / relevant rows are taken out of the first non-empty bucket (the
// row remove_first drops).  Limits ascend, so ONE running numerator S serves all of them: a limit is settled at the bucket that cuts
// it, on a bucket boundary, or at the end.  The outputs are `scale` times this walk's values, stored, or with `merge` added to what an
// earlier walk (the other kind of dropped row) has stored.  Lane t < nk accumulates the expected hits at depth k[t] on the way.
// Everything but my_k and hits is wave-uniform.
__device__ void expected_walk(const uint2 *__restrict__ cnt, int nb, uint32_t dn, uint32_t dr, const RankLimits &lims, int nlim,
                              uint32_t my_k, int nk, uint64_t tot_rel, double scale, bool merge, int64_t Qn, int64_t qi, int lane,
                              const ExpectedOut &o) {
    uint64_t B = 0, K = 0;   // rows / relevant rows ranked before the bucket
    double S = 0.0, hits = 0.0;
    int lcur = 0;
    bool first = true;
    auto put = [&](int l, double e) {
        if (lane == 0) {
            const size_t at = (size_t)l * Qn + qi;
            const double v = scale * e;
            o.ap[at] = merge ? o.ap[at] + v : v;
        }
    };
    for (int d = 0; d < nb; ++d) {
        const uint2 v = cnt[d];
        uint32_t n = v.x, r = min(v.y, v.x);
        if (n == 0u) continue;
        if (first) {
            n -= dn;
            r -= dr;
            first = false;
            if (n == 0u) continue;
        }
        if (lane < nk) {   // take_d r_d / n_d with take_d = clamp(k - B, 0, n_d); a bucket inside k whole adds r_d exactly
            const uint64_t tk = (uint64_t)my_k > B ? min((uint64_t)n, (uint64_t)my_k - B) : 0u;
            hits += tk == (uint64_t)n ? (double)r : (double)tk * (double)r / (double)n;
        }
        if (lcur < nlim) {
            while (lcur < nlim && (uint64_t)limit_of(lims, lcur) < B + n) {
                const uint32_t take = (uint32_t)((uint64_t)limit_of(lims, lcur) - B);
                double e;
                if (take == 0u)
                    e = K ? S / (double)K : 0.0;   // the limit falls on the boundary in front of this bucket
                else
                    e = cut_expectation(B, K, S, n, r, take, lane);
                put(lcur, e);
                ++lcur;
            }
            if (lcur < nlim && r > 0u) {   // the bucket lies inside every remaining limit
                double L, M;
                rank_sums(B, n, lane, L, M);
                const double second = n > 1u ? ((double)(r - 1u) / (double)(n - 1u)) * M : 0.0;
                S += ((double)r / (double)n) * ((double)(K + 1u) * L + second);
            }
        }
        B += n;
        K += r;
    }
    const double e_end = K ? S / (double)K : 0.0;   // read only where a limit is left, i.e. where S ran to the end
    for (; lcur < nlim; ++lcur) put(lcur, e_end);
    if (lane < nk) {
        const size_t at = (size_t)lane * Qn + qi;
        const uint64_t tot = tot_rel - dr;
        const double h = scale * hits, rc = tot ? scale * (hits / (double)tot) : 0.0;
        o.hits[at] = merge ? o.hits[at] + h : h;
        o.recall[at] = merge ? o.recall[at] + rc : rc;
    }
}

// remove_first: the dropped rank-1 row is uniform among the n0 rows of the lowest non-empty bucket, so the result is the mixture
// ((n0 - r0) / n0) E[that bucket as (n0 - 1, r0)] + (r0 / n0) E[(n0 - 1, r0 - 1)], for AP, hits and recall alike (the recall of a
// branch divides by the relevant rows that branch has left).  A query with no row at all gives zeros.
__global__ __launch_bounds__(256) void tie_expected_kernel(const uint32_t *__restrict__ counts, int64_t Qn, int nb, RankLimits lims,
                                                           int nlim, RankKs ks, int nk, int remove_first, ExpectedOut o) {
    const int64_t qi = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (qi >= Qn) return;   // wave-uniform
    const uint2 *cnt = (const uint2 *)counts + (size_t)qi * nb;
    unsigned long long tr = 0ull;
    int dfirst = nb;
    for (int d = lane; d < nb; d += 64) {
        const uint2 v = cnt[d];
        tr += (unsigned long long)min(v.y, v.x);
        if (v.x != 0u) dfirst = min(dfirst, d);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        tr += __shfl_xor(tr, s, 64);
        dfirst = min(dfirst, __shfl_xor(dfirst, s, 64));
    }
    dfirst = __builtin_amdgcn_readfirstlane(dfirst);
    uint32_t my_k = ks.k[0];
#pragma unroll
    for (int i = 1; i < MAX_KS; ++i) my_k = (lane == i) ? ks.k[i] : my_k;
    if (!remove_first || dfirst >= nb) {
        expected_walk(cnt, nb, 0u, 0u, lims, nlim, my_k, nk, tr, 1.0, false, Qn, qi, lane, o);
        return;
    }
    const uint2 v0 = cnt[dfirst];
    const uint32_t n0 = v0.x, r0 = min(v0.y, v0.x);
    const bool can_irr = n0 > r0, can_rel = r0 > 0u;
    if (can_irr) expected_walk(cnt, nb, 1u, 0u, lims, nlim, my_k, nk, tr, (double)(n0 - r0) / (double)n0, false, Qn, qi, lane, o);
    if (can_rel) expected_walk(cnt, nb, 1u, 1u, lims, nlim, my_k, nk, tr, (double)r0 / (double)n0, can_irr, Qn, qi, lane, o);
}

}  // namespace

extern "C" int ch_hamming_tie_expected(const uint32_t *bucket_counts, int64_t Qn, int32_t nb, const int64_t *rank_limits,
                                       int32_t nlimits, const int64_t *ks, int32_t nk, int32_t remove_first, double *out_ap,
                                       double *out_hits, double *out_recall, void *stream) {
    CH_REQUIRE(nlimits >= 0 && nlimits <= MAX_LIMITS && (nlimits == 0 || rank_limits != nullptr), "hamming_tie_expected: 0 <= nlimits <= 16");
    CH_REQUIRE(nk >= 0 && nk <= MAX_KS && (nk == 0 || ks != nullptr), "hamming_tie_expected: 0 <= nk <= 16");
    CH_REQUIRE(Qn >= 0 && nb >= 1 && nb <= 257, "hamming_tie_expected: bad sizes (nb = 64 W + 1, W <= 4)");
    if (Qn == 0 || (nlimits == 0 && nk == 0)) return 0;
    CH_REQUIRE(bucket_counts && (nlimits == 0 || out_ap) && (nk == 0 || (out_hits && out_recall)), "hamming_tie_expected: null pointer");
    CH_REQUIRE((((uintptr_t)bucket_counts | (uintptr_t)out_ap | (uintptr_t)out_hits | (uintptr_t)out_recall) & 7u) == 0,
               "hamming_tie_expected: bucket_counts (read as pairs), out_ap, out_hits and out_recall must be 8-byte aligned");
    RankLimits lims;
    if (nlimits > 0) {
        if (int e = fill_limits("hamming_tie_expected", rank_limits, nlimits, lims)) return e;
    } else {
        for (int i = 0; i < MAX_LIMITS; ++i) lims.lim[i] = 0xFFFFFFFFu;
    }
    RankKs rk;
    for (int i = 0; i < MAX_KS; ++i) {
        const int64_t k = i < nk ? ks[i] : 1;
        CH_REQUIRE(k >= 1, "hamming_tie_expected: k must be >= 1");
        rk.k[i] = k >= 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)k;
    }
    ExpectedOut o{out_ap, out_hits, out_recall};
    hipLaunchKernelGGL(tie_expected_kernel, dim3((unsigned)ceil_div64(Qn, 4)), dim3(256), 0, (hipStream_t)stream, bucket_counts, Qn,
                       (int)nb, lims, (int)nlimits, rk, (int)nk, (int)remove_first, o);
    CH_LAUNCH_CHECK();
    return 0;
}
