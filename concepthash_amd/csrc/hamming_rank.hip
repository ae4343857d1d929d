// Ranked lists of any depth on packed codes (gfx950): the pass that WRITES the gallery rows out at their rank.
//
// Replaces what a caller of the un-vendored utils.hashing builds from a full argsort of the (Qn, G) distance matrix (the first K
// hits for K beyond the top-k scan's 128, "all rows within Hamming radius r": hash lookup).  Definition:
// ascending (distance, gallery index), oracle/hamming_oracle.c `rank_one`.
//
// ch_hamming_hist counts the rows of every (segment, query, distance) bucket, ch_hamming_hist_prefix turns the counts into "rows
// ranked before" bases in ranking order (bucket, then segment).  This pass walks the gallery once more, in the work layout of those
// passes (hamming.hip: one LANE per QUERY, the gallery segment wave-uniform and walked in order, grid = query tiles x segments),
// with the tile's counters in LDS [64 W + 1][BLK] STARTING AT THE BASES instead of at zero: the value a returning ds_add hands back
// is then the row's global 0-based rank itself, and a row whose rank lies under its query's limit leaves (row, distance) in slot
// `rank` of the query's list.  One lane walks its segment in gallery order, so rows of equal distance come out in gallery order.
// Top-K of any K and "every row within radius r" are the same launch under different per-query limits.
//
// Bases ascend with the bucket, so a lane knows, once it holds them, the first bucket whose base has reached its limit (`cut`):
// no row at or beyond it can rank inside the limit, and such a row costs a distance and a compare -- with K << G nearly all do.
#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "hamming_shared.h"

namespace {

// The gallery arrives by scalar loads, UB rows per trip with the next trip's block requested before this one is consumed (the
// scalar form of the mAP passes); counters and stores are per-lane vector operations.  The counters take 66 .. 132 KB of LDS, so a CU
// holds one workgroup, one wave per SIMD, and only the block in flight hides the scalar loads' latency: eight rows per trip where two
// blocks of them fit the SGPRs (W <= 2: 2 x 32), four above.
template <int W, int BLK>
__global__ __launch_bounds__(BLK) void rank_scatter_kernel(const uint64_t *__restrict__ q, int64_t Qn, const uint64_t *__restrict__ g,
                                                           int64_t G, int seg_rows, const uint32_t *__restrict__ base,
                                                           const int64_t *__restrict__ out_start,
                                                           const uint32_t *__restrict__ out_limit, int64_t g_index_base,
                                                           int64_t *__restrict__ out_idx, int32_t *__restrict__ out_dist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cnt[];  // [NB][BLK]
    constexpr int NB = scan_buckets(W);
    constexpr int UB = W <= 2 ? 8 : 4;
    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * BLK;
    const int64_t qi = q0 + tid;
    const int seg = blockIdx.y;
    const int64_t g0 = (int64_t)seg * seg_rows;
    const int n = (int)min((int64_t)seg_rows, G - g0);
    const bool valid = qi < Qn;
    uint32_t qw[2 * W];
    load_query<W>(qw, q, qi, Qn);
    const uint32_t limit = valid ? out_limit[qi] : 0u;
    const int64_t start = valid ? out_start[qi] : 0;

    // counters = base[seg][q][bucket][0]: element e of this tile's [nq][NB] block is read by thread e % BLK (coalesced 8-byte
    // loads, the transposed form of the histogram pass's write).  Columns past Qn stay unset: their lanes never reach a counter.
    {
        const int nq = (int)min((int64_t)BLK, Qn - q0);
        const uint2 *b = (const uint2 *)(base + ((size_t)seg * Qn + q0) * NB * 2);
        for (int e = tid; e < nq * NB; e += BLK) {
            const int ql = e / NB, d = e - ql * NB;
            cnt[d * BLK + ql] = b[e].x;
        }
    }
    __syncthreads();  // each lane only touches its own column afterwards
    uint32_t *col = cnt + tid;
    uint32_t cut = 0;  // buckets [0, cut) hold a base under the limit; a lane past Qn (limit 0) keeps 0 and skips every row
    if (valid)
        for (int d = 0; d < NB; ++d) cut += col[d * BLK] < limit ? 1u : 0u;   // bases ascend with d: a count is the first index

    int64_t *oi = out_idx + start;
    int32_t *od = out_dist + start;
    const int64_t row0 = g_index_base + g0;
    auto place = [&](uint32_t d, int j) {
        if (d < cut) {
            const uint32_t rank = atomicAdd(col + d * BLK, 1u);   // rows ranked before this one
            if (rank < limit) {
                oi[rank] = row0 + j;
                od[rank] = (int32_t)d;
            }
        }
    };

    const uint64_t *__restrict__ gp = g + g0 * W;
    uint64_t bufA[UB * W], bufB[UB * W];
    auto load_block = [&](uint64_t (&dst)[UB * W], int r0) {
#pragma unroll
        for (int t = 0; t < UB * W; ++t) dst[t] = gp[(size_t)r0 * W + t];
    };
    auto scan_block = [&](const uint64_t (&blk)[UB * W], int r0) {
        uint32_t d[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) d[u] = (uint32_t)hamming<W>(qw, blk + u * W);
        // one test per trip in front of the rows' own: the trip's smallest distance against the cut, over the wave.  With K << G most
        // trips hold no row under any lane's cut and end here, at a v_min3 per two rows instead of a compare and a branch per row.
        uint32_t least = d[0];
#pragma unroll
        for (int u = 1; u < UB; ++u) least = min(least, d[u]);
        if (__builtin_amdgcn_ballot_w64(least < cut) == 0ull) return;
#pragma unroll
        for (int u = 0; u < UB; ++u) place(d[u], r0 + u);   // in row order: two rows of a trip may share a bucket
    };
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
    for (; j < n; ++j) place((uint32_t)hamming<W>(qw, gp + (size_t)j * W), j);
}

}  // namespace

extern "C" int ch_hamming_rank_scatter(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t seg_rows,
                                       const uint32_t *base, const int64_t *out_start, const uint32_t *out_limit,
                                       int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *stream) {
    CH_REQUIRE(W >= 1 && W <= 4, "hamming_rank_scatter: 1 <= W <= 4 (nbit <= 256)");
    CH_REQUIRE(seg_rows >= 1 && seg_rows <= 65535, "hamming_rank_scatter: seg_rows must be in [1, 65535]");
    CH_REQUIRE(Qn >= 0 && G >= 0, "hamming_rank_scatter: negative sizes");
    if (Qn == 0 || G == 0) return 0;
    CH_REQUIRE(q && g && base && out_start && out_limit && out_idx && out_dist, "hamming_rank_scatter: null pointer");
    CH_REQUIRE(G <= 0xFFFFFFFFll, "hamming_rank_scatter: ranks are 32-bit (G < 2^32)");
    CH_REQUIRE(ceil_div64(G, seg_rows) <= 65535, "hamming_rank_scatter: too many gallery segments (raise seg_rows)");
    return dispatch_w(W, [&](auto w) {
        constexpr int Wc = decltype(w)::value, BLK = scan_lanes(Wc);
        const size_t lds = sizeof(uint32_t) * scan_buckets(Wc) * BLK;
        dim3 grid((unsigned)ceil_div64(Qn, BLK), (unsigned)ceil_div64(G, seg_rows));
        static ch_once_per_device lds_once;   // one per instance of this body, i.e. per kernel
        if (int e = ch_func_max_lds((const void *)rank_scatter_kernel<Wc, BLK>, (int)lds, lds_once)) return e;
        hipLaunchKernelGGL((rank_scatter_kernel<Wc, BLK>), grid, dim3(BLK), lds, (hipStream_t)stream, q, Qn, g, G, seg_rows, base, out_start,
                           out_limit, g_index_base, out_idx, out_dist);
        CH_LAUNCH_CHECK();
        return 0;
    });
}
