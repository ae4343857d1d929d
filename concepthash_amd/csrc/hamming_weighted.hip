// Weighted (asymmetric) Hamming top-k (gfx950): the gallery stays binary, the query pays w_j for a disagreement on bit j, with w_j its
// own |code_j| quantised to P = 4 or 8 bits ("weighted distance"):
//     D(i, g) = sum_j w_ij [bit_j(q_i) != bit_j(g)] = sum_p 2^p popcount((q_i ^ g) & planes[i, p]),  planes[i, p] = bit p of every w_ij.
// All integers, so any segmentation or sharding of the gallery gives the same bits.
//
//  * weight_planes_kernel: codes (+ optional mask) -> planes [Qn, P, W] and wsum [Qn] = the largest D a query can reach.
//  * topk_weighted_partial_kernel<W, KREG, P>: the scan of topk_partial_kernel (hamming.hip) -- one lane per query, the gallery
//    segment wave-uniform through scalar loads in two alternating four-row buffers, a ballot-gated branch-free insertion network --
//    with one popcount accumulator per plane, chained across the words, and a Horner chain of P - 1 shift-adds at the end of a row.
//    key = D << 16 | row-in-segment: D <= 255 * 256 = 65,280 < 2^16 - 1, so 0xFFFFFFFF stays the empty slot; segments hold <= 65,536 rows.
//  * the merge is the one of the unweighted scan with the key split at bit 16 (hamming_shared.h).
#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "hamming_shared.h"

namespace {

constexpr int WKEY_SHIFT = 16;
constexpr int64_t WSEG_MAX_ROWS = 1 << WKEY_SHIFT;

// ---------------------------------------------------------------------------------------------------------------
// quantised weights -> bit planes
// ---------------------------------------------------------------------------------------------------------------
// One wave per query; lane b holds bit b of every 64-bit word (W <= 4 values).  a = |c| (0 where c is not finite, the bit is masked
// out or past nbit); amax by wave shuffles; w = floor(a L / amax + 0.5) in fp64 on the widened fp32 values (a L is exact, the IEEE
// quotient and the sum round as the host's do); plane p of word t is the 64-lane ballot of bit p of w.
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
// the scan
// ---------------------------------------------------------------------------------------------------------------
// key = D << 16 | row with the (wave-uniform) row number taken from an SGPR: one v_lshl_or_b32
__device__ __forceinline__ uint32_t make_wkey(uint32_t d, uint32_t row_uniform) {
    uint32_t key;
    asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(key) : "v"(d), "n"(WKEY_SHIFT), "s"(row_uniform));
    return key;
}

// D of one gallery row: per 32-bit word and plane one (q ^ g) & plane (a single v_bitop3_b32 with the gallery word as its SGPR
// operand) and one chained v_bcnt into that plane's accumulator -- 2 P instructions per word -- then P - 1 shift-adds
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
    uint32_t d = acc[P - 1];
#pragma unroll
    for (int p = P - 2; p >= 0; --p) d = (d << 1) + acc[p];
    return d;
}

template <int W, int KREG, int P>
__global__ __launch_bounds__(256) void topk_weighted_partial_kernel(const uint64_t *__restrict__ q,
                                                                    const uint64_t *__restrict__ planes, int64_t Qn,
                                                                    const uint64_t *__restrict__ g, int64_t G, int seg_rows, int k,
                                                                    uint32_t *__restrict__ part) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int seg = blockIdx.y;
    const int64_t g0 = (int64_t)seg * seg_rows;
    const int n = (int)min((int64_t)seg_rows, G - g0);
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
    // four gallery rows per trip: one wide scalar load (the next block is requested before this one is consumed), four keys, ONE
    // threshold test on their minimum; the insertion network runs only if some lane beats its list.
    constexpr int UB = 4;
    uint64_t bufA[UB * W], bufB[UB * W];
    auto load_block = [&](uint64_t (&dst)[UB * W], int row) {
#pragma unroll
        for (int t = 0; t < UB * W; ++t) dst[t] = gp[(size_t)row * W + t];
    };
    auto scan_block = [&](const uint64_t (&blk)[UB * W], int row) {
        uint32_t key[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) key[u] = make_wkey(weighted_dist<W, P>(qw, pl, blk + u * W), (uint32_t)(row + u));
        const uint32_t kmin = min(min(key[0], key[1]), min(key[2], key[3]));
        if (__builtin_amdgcn_ballot_w64(kmin < list[KREG - 1]) != 0ull) {
#pragma unroll
            for (int u = 0; u < UB; ++u) insert(key[u]);
        }
    };
    // two blocks per iteration with the two SGPR buffers taking turns: no register copies between trips
    int j = 0;
    if (n >= UB) load_block(bufA, 0);
    for (; j + 2 * UB <= n; j += 2 * UB) {
        load_block(bufB, j + UB);
        scan_block(bufA, j);
        if (j + 3 * UB <= n) load_block(bufA, j + 2 * UB);
        scan_block(bufB, j + UB);
    }
    if (j + UB <= n) {  // an odd number of whole blocks: the last one is already in bufA
        scan_block(bufA, j);
        j += UB;
    }
    for (; j < n; ++j) insert((weighted_dist<W, P>(qw, pl, gp + (size_t)j * W) << WKEY_SHIFT) | (uint32_t)j);
    if (qi < Qn) {
        uint32_t *o = part + ((size_t)seg * Qn + qi) * k;
#pragma unroll
        for (int i = 0; i < KREG; ++i)
            if (i < k) o[i] = list[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
// VGPRs of topk_weighted_partial_kernel<W, KREG, P> from the code-object metadata of this build (profiles/search_weighted_topk.txt;
// no instance uses scratch).  The kernel has no LDS, so a CU holds min(8, 512 / VGPRs rounded up to the allocation unit of 8)
// workgroups of four waves.
constexpr int WTOPK_VGPRS[2][4][5] = {
    // KREG 10, 16, 32, 64, 128
    {{32, 44, 76, 140, 258}, {43, 54, 86, 150, 258}, {53, 64, 96, 160, 258}, {63, 74, 106, 170, 258}},     // P = 4, W = 1..4
    {{47, 53, 84, 148, 258}, {67, 73, 102, 166, 258}, {85, 91, 120, 184, 258}, {103, 109, 138, 202, 266}},  // P = 8, W = 1..4
};

int wtopk_seg_rows(int64_t Qn, int64_t G, int W, int k, int P) {
    const int ki = k <= 10 ? 0 : k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 3 : 4;
    const int vgprs = (WTOPK_VGPRS[P == 8][W - 1][ki] + 7) / 8 * 8;
    const int per_cu = std::max(1, std::min(8, 512 / std::max(8, vgprs)));
    return topk_seg_rows_for(Qn, G, per_cu, WSEG_MAX_ROWS);
}

template <int W, int KREG, int P>
int launch_wtopk_partial(const uint64_t *q, const uint64_t *planes, int64_t Qn, const uint64_t *g, int64_t G, int seg_rows, int k,
                         uint32_t *part, hipStream_t s) {
    const int nseg = (int)ceil_div64(G, seg_rows);
    dim3 grid((unsigned)ceil_div64(Qn, 256), (unsigned)nseg);
    hipLaunchKernelGGL((topk_weighted_partial_kernel<W, KREG, P>), grid, dim3(256), 0, s, q, planes, Qn, g, G, seg_rows, k, part);
    CH_LAUNCH_CHECK();
    return 0;
}

template <int W, int P>
int wtopk_dispatch_k(const uint64_t *q, const uint64_t *planes, int64_t Qn, const uint64_t *g, int64_t G, int seg_rows, int k,
                     uint32_t *part, hipStream_t s) {
    if (k <= 10) return launch_wtopk_partial<W, 10, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
    if (k <= 16) return launch_wtopk_partial<W, 16, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
    if (k <= 32) return launch_wtopk_partial<W, 32, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
    if (k <= 64) return launch_wtopk_partial<W, 64, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
    return launch_wtopk_partial<W, 128, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
}

template <int P>
int wtopk_dispatch_w(const uint64_t *q, const uint64_t *planes, int64_t Qn, const uint64_t *g, int64_t G, int W, int seg_rows, int k,
                     uint32_t *part, hipStream_t s) {
    switch (W) {
        case 1: return wtopk_dispatch_k<1, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
        case 2: return wtopk_dispatch_k<2, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
        case 3: return wtopk_dispatch_k<3, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
        default: return wtopk_dispatch_k<4, P>(q, planes, Qn, g, G, seg_rows, k, part, s);
    }
}

}  // namespace

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

extern "C" size_t ch_hamming_topk_weighted_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k) {
    if (Qn <= 0 || G <= 0 || k <= 0 || W < 1 || W > 4) return 16;
    // the call does not name P: room for the finer of the two segmentations
    const int rows = std::min(wtopk_seg_rows(Qn, G, W, k, 4), wtopk_seg_rows(Qn, G, W, k, 8));
    return (size_t)(ceil_div64(G, rows) * Qn * k) * sizeof(uint32_t) + 16;
}

extern "C" int ch_hamming_topk_weighted(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                                        int32_t W, int32_t k, int64_t g_index_base, int64_t *out_idx, int32_t *out_dist,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    CH_REQUIRE(P == 4 || P == 8, "hamming_topk_weighted: P (weight bits) must be 4 or 8");
    CH_REQUIRE(W >= 1 && W <= 4, "hamming_topk_weighted: 1 <= W <= 4 (nbit <= 256)");
    CH_REQUIRE(k >= 1 && k <= 128, "hamming_topk_weighted: 1 <= k <= 128");
    CH_REQUIRE(Qn >= 0 && G >= 0, "hamming_topk_weighted: negative sizes");
    if (Qn == 0) return 0;
    CH_REQUIRE(q && planes && out_idx && out_dist, "hamming_topk_weighted: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (G == 0) {
        CH_CHECK_HIP(hipMemsetAsync(out_idx, 0xFF, sizeof(int64_t) * Qn * k, s));
        CH_CHECK_HIP(hipMemsetAsync(out_dist, 0xFF, sizeof(int32_t) * Qn * k, s));
        return 0;
    }
    CH_REQUIRE(g != nullptr, "hamming_topk_weighted: null gallery");
    const int seg_rows = wtopk_seg_rows(Qn, G, W, k, P);
    const int64_t nseg = ceil_div64(G, seg_rows);
    CH_REQUIRE(nseg <= 65535, "hamming_topk_weighted: gallery too large for one call: more than 65,535 segments (shard it)");
    CH_REQUIRE(workspace && workspace_bytes >= ch_hamming_topk_weighted_workspace(Qn, G, W, k),
               "hamming_topk_weighted: workspace too small");
    uint32_t *part = (uint32_t *)workspace;
    const int e = P == 4 ? wtopk_dispatch_w<4>(q, planes, Qn, g, G, W, seg_rows, k, part, s)
                         : wtopk_dispatch_w<8>(q, planes, Qn, g, G, W, seg_rows, k, part, s);
    if (e) return e;
    hipLaunchKernelGGL(topk_merge_keys_kernel<WKEY_SHIFT>, dim3((unsigned)ceil_div64(Qn, 4)), dim3(256), 0, s, part, (int)nseg, Qn, (int)k, seg_rows,
                       g_index_base, out_idx, out_dist);
    CH_LAUNCH_CHECK();
    return 0;
}
