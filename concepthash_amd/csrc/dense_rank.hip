// Real-valued codes (gfx950): the rankings by cosine, squared Euclidean and dot distance of the codes before sign() -- prepare,
// distance matrix, exact top-k and the rank-counting evaluation ("real-valued codes").  Built with
// -ffp-contract=off: every multiply-add below is an fmaf that is written down.
//
// The scan operand ("prepared" codes, ch_dense_prepare): rows in blocks of 64, dimension-major inside a block,
//     prepared[(r / 64) * n * 64 + j * 64 + r % 64] = x^_r,j        (x^ = x, or x / |x| for cosine; rows past the end of the last block: zeros)
// so the 64 lanes of a wave that own 64 consecutive rows load dimension j with one contiguous 256-byte access, and dimension j of 16
// consecutive queries is one contiguous 64-byte scalar load.  Queries and gallery are prepared alike.
//
// The distance is ONE function, dense_tile<M, TQ>: TQ queries (wave-uniform: their values reach the fmaf as its scalar operand)
// against one row per lane; for every (query, row) pair the chain
//     acc = 0.0f;  for j = 0 .. n - 1 in this order:   dot, cosine: acc = fmaf(q_j, g_j, acc)     euclidean: t = q_j - g_j; acc = fmaf(t, t, acc)
//     D = -acc + 0.0f (dot)      1.0f - acc + 0.0f (cosine)      acc + 0.0f (euclidean)              (+ 0.0f: -0 becomes +0)
// The distance matrix (TQ = 1, one pair per lane), the top-k scan (TQ = 16), the collect pass (TQ = 1, relevant pairs only) and the
// count pass (TQ = 1) all call it, so D(q, g) has the same bits in every pass whatever the tile or the segmentation -- a rank-counting
// evaluation ranks a relevant row against its own collected key, and one ulp between two passes would move a rank by one.  No MFMA.
//
// Order: ord(D) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), b = bits(D), ascending as unsigned as D ascends; every ranking is ascending
// key = ord(D) << 32 | row index, the key layout of the other rank-counting evaluations (hamming_shared.h).
//
// Top-k: one workgroup per (tile of 16 queries, gallery segment), lanes own gallery rows.  Per query of the tile LDS holds a threshold
// (a 64-bit key; at first above every key), a fill count and DT_CAP = 384 candidate keys.  A trip is 256 rows: a lane appends the key
// of its row to the lists of the queries whose threshold it is below.  After a trip, every list longer than min(128, 4 k) is cut by
// the whole workgroup to its k smallest, in order (each key's rank = the number of keys below it: keys are distinct), and the k-th
// becomes the threshold; a list is at most 128 long before a trip, so 256 appends fit.  Segment lists are merged by one wave per query.
//
// Rerank (ch_dense_rerank): the same distance over a shortlist of rows per query, read from the RAW row-major codes -- see there.
#include <algorithm>
#include <string>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "hamming_shared.h"

namespace {

constexpr int DM_COSINE = 0, DM_EUCLIDEAN = 1, DM_DOT = 2;
constexpr int DB = 64;   // rows of a block of the prepared layout

__host__ __device__ __forceinline__ int64_t prepared_floats(int64_t rows, int n) { return (rows + DB - 1) / DB * DB * n; }

// ---------------------------------------------------------------------------------------------------------------
// the distance
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ float dense_step(float q, float g, float acc) {
    if constexpr (M == DM_EUCLIDEAN) {
        const float t = q - g;
        return fmaf(t, t, acc);
    } else {
        return fmaf(q, g, acc);
    }
}

template <int M>
__device__ __forceinline__ float dense_finish(float acc) {
    if constexpr (M == DM_EUCLIDEAN) return acc + 0.0f;
    if constexpr (M == DM_COSINE) return (1.0f - acc) + 0.0f;
    return (-acc) + 0.0f;
}

// qp: dimension 0 of the tile's first query, gp: dimension 0 of the lane's row, both inside their blocks (dimension j: + j * 64)
template <int M, int TQ>
__device__ __forceinline__ void dense_tile(const float *__restrict__ qp, const float *__restrict__ gp, int n, float (&D)[TQ]) {
    float acc[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) acc[t] = 0.0f;
    auto dim = [&](int j) {
        const float g = gp[(size_t)j * DB];
#pragma unroll
        for (int t = 0; t < TQ; ++t) acc[t] = dense_step<M>(qp[(size_t)j * DB + t], g, acc[t]);
    };
    // a tile of queries keeps its lanes busy with 4 dimensions in flight; one query per lane wants more loads out at a time
    if constexpr (TQ == 1) {
#pragma unroll 16
        for (int j = 0; j < n; ++j) dim(j);
    } else {
#pragma unroll 4
        for (int j = 0; j < n; ++j) dim(j);
    }
#pragma unroll
    for (int t = 0; t < TQ; ++t) D[t] = dense_finish<M>(acc[t]);
}

__device__ __forceinline__ const float *row_ptr(const float *p, int64_t r, int n) { return p + (r >> 6) * (int64_t)n * DB + (r & 63); }

__device__ __forceinline__ uint32_t dense_ord(float D) {
    const uint32_t b = __builtin_bit_cast(uint32_t, D);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float dense_unord(uint32_t o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// f(std::integral_constant<int, M>) for a checked metric id
template <class F>
int dispatch_metric(int metric, F &&f) {
    switch (metric) {
        case DM_COSINE: return f(std::integral_constant<int, DM_COSINE>{});
        case DM_EUCLIDEAN: return f(std::integral_constant<int, DM_EUCLIDEAN>{});
        default: return f(std::integral_constant<int, DM_DOT>{});
    }
}

// The cosine scale of one row-major row: 1 / |x| by the chain s = fmaf(x_j, x_j, s) from 0.0f over j = 0 .. n - 1, 0 for a zero row.  A
// normalised entry is x_j * scale, rounded on its own.  Prepare and the rerank both normalise through here, so a row has the same
// normalised bits in the prepared operand and on the fly.  A pass that meets a row piece by piece (the staged rerank) walks the same
// chain through dense_sq_step and ends it with dense_scale_of.
__device__ __forceinline__ float dense_sq_step(float x, float s) { return fmaf(x, x, s); }
__device__ __forceinline__ float dense_scale_of(float s) { return s == 0.0f ? 0.0f : __fdiv_rn(1.0f, __fsqrt_rn(s)); }
__device__ __forceinline__ float dense_row_scale(const float *__restrict__ x, int n) {
    float s = 0.0f;
    for (int j = 0; j < n; ++j) s = dense_sq_step(x[j], s);
    return dense_scale_of(s);
}

// ---------------------------------------------------------------------------------------------------------------
// prepare: one lane per row of the padded operand
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dense_prepare_kernel(const float *__restrict__ codes, int64_t rows, int n, int metric,
                                                            float *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (rows + DB - 1) / DB * DB) return;
    float *o = out + (r >> 6) * (int64_t)n * DB + (r & 63);
    if (r >= rows) {
        for (int j = 0; j < n; ++j) o[(size_t)j * DB] = 0.0f;
        return;
    }
    const float *x = codes + r * n;
    const float scale = metric == DM_COSINE ? dense_row_scale(x, n) : 1.0f;
    if (metric == DM_COSINE)
        for (int j = 0; j < n; ++j) o[(size_t)j * DB] = x[j] * scale;
    else
        for (int j = 0; j < n; ++j) o[(size_t)j * DB] = x[j];
}

// ---------------------------------------------------------------------------------------------------------------
// the distance matrix: one pair per lane
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(256) void dense_dist_kernel(const float *__restrict__ q, int64_t Qn, const float *__restrict__ g, int64_t G,
                                                         int n, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= Qn * G) return;
    const int64_t qi = t / G, j = t - qi * G;
    float D[1];
    dense_tile<M, 1>(row_ptr(q, qi, n), row_ptr(g, j, n), n, D);
    out[t] = D[0];
}

// ---------------------------------------------------------------------------------------------------------------
// top-k
// ---------------------------------------------------------------------------------------------------------------
constexpr int DT_TQ = 16;      // queries of a tile (16 divides 64: a tile lies inside one block)
constexpr int DT_BLK = 256;    // lanes of a workgroup = rows of a trip
constexpr int DT_KMAX = 128;
constexpr int DT_CAP = DT_KMAX + DT_BLK;   // keys a query's list can hold: at most 128 before a trip, which appends at most 256
constexpr uint64_t DT_EMPTY = ~0ull;       // ord = 0xFFFFFFFF is a NaN's: no finite distance has it

// cut list t to its k smallest keys, ascending; called by the whole workgroup with c = the list's fill, the same value in every lane
__device__ __forceinline__ void dense_cut(uint64_t *list, uint32_t c, int k, uint64_t *thr, uint32_t *cnt) {
    const int tid = threadIdx.x;
    uint64_t key[2];
    uint32_t rank[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const uint32_t i = tid + e * DT_BLK;
        key[e] = i < c ? list[i] : DT_EMPTY;
        rank[e] = 0u;
    }
    for (uint32_t i = 0; i < c; ++i) {
        const uint64_t other = list[i];
        rank[0] += other < key[0] ? 1u : 0u;
        rank[1] += other < key[1] ? 1u : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (tid + e * DT_BLK < (int)c && rank[e] < (uint32_t)k) {
            list[rank[e]] = key[e];
            if (rank[e] == (uint32_t)k - 1u) *thr = key[e];
        }
    }
    if (tid == 0) *cnt = min(c, (uint32_t)k);
    __syncthreads();
}

template <int M>
__global__ __launch_bounds__(DT_BLK) void dense_topk_partial_kernel(const float *__restrict__ q, int64_t Qn, const float *__restrict__ g,
                                                                    int64_t G, int n, int seg_rows, int k, uint64_t *__restrict__ part) {
    __shared__ uint64_t cand[DT_TQ][DT_CAP];
    __shared__ uint64_t thr[DT_TQ];
    __shared__ uint32_t cnt[DT_TQ];
    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * DT_TQ;
    const int seg = blockIdx.y;
    const int64_t g0 = (int64_t)seg * seg_rows;
    const int nrows = (int)min((int64_t)seg_rows, G - g0);
    if (tid < DT_TQ) {
        thr[tid] = DT_EMPTY;
        cnt[tid] = 0u;
    }
    __syncthreads();
    const float *qp = row_ptr(q, q0, n);   // queries past Qn inside the last block are zero rows: scanned, never stored
    const uint32_t lim = (uint32_t)min(DT_KMAX, 4 * k);
    for (int r0 = 0; r0 < nrows; r0 += DT_BLK) {   // the same trips for every lane: the barriers below are a workgroup's
        const int r = r0 + tid;
        const bool valid = r < nrows;
        const int64_t row = g0 + (valid ? r : 0);
        float D[DT_TQ];
        dense_tile<M, DT_TQ>(qp, row_ptr(g, row, n), n, D);
#pragma unroll
        for (int t = 0; t < DT_TQ; ++t) {
            const uint64_t key = ((uint64_t)dense_ord(D[t]) << 32) | (uint64_t)row;
            if (valid && key < thr[t]) cand[t][atomicAdd(&cnt[t], 1u)] = key;
        }
        __syncthreads();
        for (int t = 0; t < DT_TQ; ++t) {
            const uint32_t c = cnt[t];   // the same value in every lane: nobody appends before the next trip
            if (c > lim) dense_cut(cand[t], c, k, &thr[t], &cnt[t]);
        }
        __syncthreads();   // every lane has read every fill before the next trip appends
    }
    for (int t = 0; t < DT_TQ; ++t) {
        const uint32_t c = cnt[t];
        dense_cut(cand[t], c, k, &thr[t], &cnt[t]);
        const int64_t qi = q0 + t;
        if (qi < Qn && tid < k) part[((size_t)seg * Qn + qi) * k + tid] = tid < (int)min(c, (uint32_t)k) ? cand[t][tid] : DT_EMPTY;
    }
}

// one wave per query: repeatedly extract the smallest key above the previous one (keys are distinct: they hold the row)
__global__ __launch_bounds__(256) void dense_topk_merge_kernel(const uint64_t *__restrict__ part, int nseg, int64_t Qn, int k,
                                                               int64_t g_index_base, int64_t *__restrict__ out_idx,
                                                               float *__restrict__ out_dist) {
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (qi >= Qn) return;
    const int ncand = nseg * k;
    bool any = false;
    uint64_t prev = 0ull;   // the last output, once there is one
    for (int r = 0; r < k; ++r) {
        uint64_t best = DT_EMPTY;
        for (int c = lane; c < ncand; c += 64) {
            const int s = c / k, i = c - s * k;
            const uint64_t key = part[((size_t)s * Qn + qi) * k + i];
            if ((!any || key > prev) && key < best) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)best, o, 64);
            best = other < best ? other : best;
        }
        if (best == DT_EMPTY) {   // nothing left: fill the rest
            for (int rr = r + lane; rr < k; rr += 64) {
                out_idx[qi * k + rr] = -1;
                out_dist[qi * k + rr] = __builtin_inff();
            }
            return;
        }
        if (lane == 0) {
            out_idx[qi * k + r] = g_index_base + (int64_t)(best & 0xFFFFFFFFull);
            out_dist[qi * k + r] = dense_unord((uint32_t)(best >> 32));
        }
        prev = best;
        any = true;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// rerank: the second stage of a two-stage search ("two-stage").  One workgroup per query; the codes are the raw
// row-major ones, so a candidate row is one contiguous read.  The query goes into LDS once (normalised there for cosine, by
// dense_row_scale and x * scale as prepare does it); a lane owns a candidate and walks its row against the query -- every lane reads
// the same query entry: an LDS broadcast -- through dense_step / dense_finish over j = 0 .. n - 1, and leaves key = ord(D) << 32 | row
// in LDS.  An empty slot (id < 0 or row outside [0, G)) is never dereferenced and leaves DT_EMPTY.  The P = 2^ceil(log2 m) keys (the
// pad is DT_EMPTY) are sorted by a bitonic network, and the first k go out.
// How a lane gets its row.  WIDE (n a multiple of 4, a 16-byte aligned plane): a trip takes 256 candidates, and their rows come through
// an LDS tile in chunks of RR_DC = 16 dimensions -- four lanes load the 64 bytes of one row's chunk with one 16-byte load each, so a
// wave's load instruction covers 16 rows in whole 64-byte pieces instead of 64 rows in 16-byte ones; a lane then reads its own row's
// chunk from the tile (row stride 17 floats: the 64 lanes of a wave read 64 different banks).  cosine sweeps the row twice, first for
// the scale.  Otherwise a lane reads its row from global memory with scalar loads.
// ---------------------------------------------------------------------------------------------------------------
constexpr int RR_BLK = 256;
constexpr int RR_MAX = 4096;      // candidates per query: 32 KB of keys
constexpr int RR_DC = 16;         // dimensions of a staged chunk
constexpr int RR_TS = RR_DC + 1;  // floats between two rows of the tile

// the distance of the LDS query qs (normalised already for cosine) to the raw row x, read where it lies
template <int M>
__device__ __forceinline__ float rerank_dist(const float *qs, const float *__restrict__ x, int n) {
    float scale = 1.0f;
    if constexpr (M == DM_COSINE) scale = dense_row_scale(x, n);
    float acc = 0.0f;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        float v = x[j];
        if constexpr (M == DM_COSINE) v = v * scale;
        acc = dense_step<M>(qs[j], v, acc);
    }
    return dense_finish<M>(acc);
}

template <int M, bool WIDE>
__global__ __launch_bounds__(RR_BLK) void dense_rerank_kernel(const float *__restrict__ q, const float *__restrict__ g, int64_t G, int n,
                                                              const int64_t *__restrict__ cand, int m, int P, int k, int64_t g_index_base,
                                                              int64_t *__restrict__ out_idx, float *__restrict__ out_dist) {
    extern __shared__ __align__(16) uint64_t rr_lds[];   // P keys, the query (256 floats) and, WIDE, the tile (256 rows of RR_TS floats)
    uint64_t *keys = rr_lds;
    float *qs = (float *)(rr_lds + P);
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    if (tid < n) qs[tid] = q[qi * n + tid];
    for (int c = tid; c < P; c += RR_BLK) keys[c] = DT_EMPTY;
    __syncthreads();
    if constexpr (M == DM_COSINE) {
        const float scale = dense_row_scale(qs, n);   // every lane walks the same chain: LDS broadcasts
        __syncthreads();
        if (tid < n) qs[tid] = qs[tid] * scale;
        __syncthreads();
    }
    for (int c0 = 0; c0 < m; c0 += RR_BLK) {   // the same trips for every lane: the barriers below are a workgroup's
        const int c = c0 + tid;
        int64_t row = -1;
        if (c < m) {
            const int64_t id = cand[qi * m + c];
            if (id >= 0 && id - g_index_base >= 0 && id - g_index_base < G) row = id - g_index_base;
        }
        float D = 0.0f;
        if constexpr (WIDE) {
            float *tile = qs + 256;
            const int lane = tid & 63, piece = (lane & 3) * 4;
            // the four rows of this wave that the lane loads a piece of: row i * 16 + lane / 4, dimensions piece .. piece + 3 of a chunk
            const float *src[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t rrow = __shfl((long long)row, i * 16 + (lane >> 2), 64);
                src[i] = rrow >= 0 ? g + rrow * n + piece : nullptr;
            }
            float4 next[4];
            auto load = [&](int d0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (src[i] && d0 + piece < n) next[i] = *(const float4 *)(src[i] + d0);
            };
            // use(j, x_j) for j = 0 .. n - 1 in this order, x the lane's own row; the loads of a chunk fly while the one before it is used
            auto sweep = [&](auto &&use) {
                load(0);
                for (int d0 = 0; d0 < n; d0 += RR_DC) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (src[i] && d0 + piece < n) {
                            float *t = tile + ((tid & ~63) + i * 16 + (lane >> 2)) * RR_TS + piece;
                            t[0] = next[i].x;
                            t[1] = next[i].y;
                            t[2] = next[i].z;
                            t[3] = next[i].w;
                        }
                    }
                    __syncthreads();
                    if (d0 + RR_DC < n) load(d0 + RR_DC);
                    if (row >= 0) {
                        const float *t = tile + tid * RR_TS;
                        const int dn = min(RR_DC, n - d0);
#pragma unroll 4
                        for (int j = 0; j < dn; ++j) use(d0 + j, t[j]);
                    }
                    __syncthreads();   // the tile is read before the next chunk overwrites it
                }
            };
            float scale = 1.0f;
            if constexpr (M == DM_COSINE) {
                float s = 0.0f;
                sweep([&](int, float v) { s = dense_sq_step(v, s); });
                scale = dense_scale_of(s);
            }
            float acc = 0.0f;
            sweep([&](int j, float v) {
                if constexpr (M == DM_COSINE) v = v * scale;
                acc = dense_step<M>(qs[j], v, acc);
            });
            D = dense_finish<M>(acc);
        } else {
            if (row >= 0) D = rerank_dist<M>(qs, g + row * n, n);
        }
        if (row >= 0) keys[c] = ((uint64_t)dense_ord(D) << 32) | (uint64_t)row;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += RR_BLK) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & size) == 0)) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int r = tid; r < k; r += RR_BLK) {
        const uint64_t key = keys[r];
        const bool empty = key == DT_EMPTY;
        out_idx[qi * k + r] = empty ? -1 : g_index_base + (int64_t)(key & 0xFFFFFFFFull);
        out_dist[qi * k + r] = empty ? __builtin_inff() : dense_unord((uint32_t)(key >> 32));
    }
}

// Rows per segment where the caller leaves it open: about three workgroups per CU (48 KB of LDS each) over the 256 CUs, segments of at
// least 4,096 rows -- every segment starts with empty lists, and its first trips cut every list -- and a multiple of the trip.
int dense_seg_rows(int64_t Qn, int64_t G) {
    const int64_t tiles = ceil_div64(Qn, DT_TQ);
    const int64_t nseg = std::max<int64_t>(1, std::min<int64_t>(ceil_div64(768, tiles), G / 4096));
    int64_t rows = round_up64(ceil_div64(G, nseg), DT_BLK);
    rows = std::max<int64_t>(rows, round_up64(ceil_div64(G, 65535), DT_BLK));
    return (int)std::min<int64_t>(rows, 0x40000000);
}

// ---------------------------------------------------------------------------------------------------------------
// evaluation by rank counting: the collect and the count pass are rank_collect_kernel and rank_count_kernel of hamming_shared.h under
// this distance, behind the shared launches and entry bodies.  The prepared gallery goes behind the pointer type of the shared kernels.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
struct DenseRow {
    const float *q;
    int n;
    // W is not used
    __device__ __forceinline__ uint32_t row(int64_t qi, int, const uint64_t *__restrict__ g, int64_t j) const {
        float D[1];
        dense_tile<M, 1>(row_ptr(q, qi, n), row_ptr((const float *)g, j, n), n, D);
        return dense_ord(D[0]);
    }
};

// What rank_count_kernel takes.  Its "registers" are the address of the query's dimension 0 and the segment; the row loop
// (dense_count_rows) takes one row per lane and trip -- a dense row does not fit rank_count_rows' two rows of registers at n = 256 --
// with its keys, list and bins.
template <int M>
struct DenseCount {
    struct Regs {
        const float *qp, *g;
        int64_t g0;
    };
    const float *q;
    int n;
    __device__ __forceinline__ void load(Regs &r, int64_t qi, const uint64_t *__restrict__ g, int64_t g0) const {
        r = Regs{row_ptr(q, qi, n), (const float *)g, g0};
    }
    __device__ __forceinline__ void rows(const Regs &s, int nrows, uint64_t row0, const uint64_t *list, uint32_t nkeys, uint64_t last,
                                         uint32_t *bins) const {
        for (int r = threadIdx.x; r < nrows; r += RC_BLK) {
            float D[1];
            dense_tile<M, 1>(s.qp, row_ptr(s.g, s.g0 + r, n), n, D);
            const uint64_t key = ((uint64_t)dense_ord(D[0]) << 32) | (row0 + (uint64_t)r);
            if (key <= last) atomicAdd(bins + keys_below(list, nkeys, key), 1u);
        }
    }
};

int check_dense(const char *who, int n, int metric) {
    const std::string at = std::string(who) + ": ";
    CH_REQUIRE(n >= 1 && n <= 256, at + "n must be in [1, 256]");
    CH_REQUIRE(metric >= 0 && metric <= 2, at + "metric must be 0 (cosine), 1 (euclidean) or 2 (dot)");
    return 0;
}

// what rank_collect_run / rank_count_run take as the ranking (W = 1 passes the shared check of W, which dense codes do not have)
struct DenseRanking {
    static constexpr const char *with_offsets = "q and keys";
    const float *q;
    int n, metric;
    int check(const char *who, int64_t Qn, int64_t G, int64_t g_index_base) const {
        if (int e = check_dense(who, n, metric)) return e;
        return check_rank_sizes(who, Qn, G, 1, g_index_base);
    }
    bool operands() const { return q != nullptr; }
    template <class F> int collect(F &&f) const { return dispatch_metric(metric, [&](auto m) { return f(DenseRow<decltype(m)::value>{q, n}, 1); }); }
    template <class F> int count(F &&f) const { return dispatch_metric(metric, [&](auto m) { return f(DenseCount<decltype(m)::value>{q, n}); }); }
};

}  // namespace

extern "C" size_t ch_dense_prepared_bytes(int64_t rows, int32_t n) {
    if (rows <= 0 || n < 1) return 0;
    return (size_t)prepared_floats(rows, n) * sizeof(float);
}

extern "C" int ch_dense_prepare(const float *codes, int64_t rows, int32_t n, int32_t metric, float *out, void *stream) {
    if (int e = check_dense("dense_prepare", n, metric)) return e;
    CH_REQUIRE(rows >= 0, "dense_prepare: negative rows");
    if (rows == 0) return 0;
    CH_REQUIRE(codes && out, "dense_prepare: null pointer");
    hipLaunchKernelGGL(dense_prepare_kernel, dim3((unsigned)ceil_div64(round_up64(rows, DB), 256)), dim3(256), 0, (hipStream_t)stream, codes,
                       rows, (int)n, (int)metric, out);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_dense_dist(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, float *out, void *stream) {
    if (int e = check_dense("dense_dist", n, metric)) return e;
    CH_REQUIRE(Qn >= 0 && G >= 0, "dense_dist: negative sizes");
    if (Qn == 0 || G == 0) return 0;
    CH_REQUIRE(q && g && out, "dense_dist: null pointer");
    CH_REQUIRE(ceil_div64(Qn * G, 256) <= 0x7FFFFFFFll, "dense_dist: Qn x G too large for one call (small problems)");
    return dispatch_metric(metric, [&](auto m) {
        hipLaunchKernelGGL((dense_dist_kernel<decltype(m)::value>), dim3((unsigned)ceil_div64(Qn * G, 256)), dim3(256), 0, (hipStream_t)stream,
                           q, Qn, g, G, (int)n, out);
        CH_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int32_t ch_dense_topk_seg_rows(int64_t Qn, int64_t G) {
    if (Qn <= 0 || G <= 0) return DT_BLK;
    return dense_seg_rows(Qn, G);
}

extern "C" size_t ch_dense_topk_workspace(int64_t Qn, int64_t G, int32_t k, int32_t seg_rows) {
    if (Qn <= 0 || G <= 0 || k <= 0) return 16;
    const int rows = seg_rows > 0 ? seg_rows : dense_seg_rows(Qn, G);
    return (size_t)(ceil_div64(G, rows) * Qn * k) * sizeof(uint64_t) + 16;
}

extern "C" int ch_dense_topk(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, int32_t k,
                             int64_t g_index_base, int32_t seg_rows, int64_t *out_idx, float *out_dist, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (int e = check_dense("dense_topk", n, metric)) return e;
    CH_REQUIRE(k >= 1 && k <= DT_KMAX, "dense_topk: 1 <= k <= 128");
    CH_REQUIRE(Qn >= 0 && G >= 0, "dense_topk: negative sizes");
    CH_REQUIRE(seg_rows >= 0, "dense_topk: seg_rows must be >= 0 (0: chosen here)");
    CH_REQUIRE(g_index_base >= 0 && g_index_base + G <= 0x100000000ll, "dense_topk: keys hold 32-bit row indices (g_index_base + G <= 2^32)");
    if (Qn == 0) return 0;
    CH_REQUIRE(q && out_idx && out_dist, "dense_topk: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int rows = seg_rows > 0 ? seg_rows : dense_seg_rows(Qn, std::max<int64_t>(G, 1));
    const int64_t nseg = ceil_div64(G, rows);
    CH_REQUIRE(nseg <= 65535, "dense_topk: gallery too large for one call: more than 65,535 segments (shard it, or raise seg_rows)");
    CH_REQUIRE(ceil_div64(Qn, DT_TQ) <= 0x7FFFFFFFll, "dense_topk: too many queries for one call");
    uint64_t *part = (uint64_t *)workspace;
    if (G > 0) {
        CH_REQUIRE(g != nullptr, "dense_topk: null gallery");
        CH_REQUIRE(workspace && workspace_bytes >= ch_dense_topk_workspace(Qn, G, k, seg_rows), "dense_topk: workspace too small");
        const dim3 grid((unsigned)ceil_div64(Qn, DT_TQ), (unsigned)nseg);
        if (int e = dispatch_metric(metric, [&](auto m) {
                hipLaunchKernelGGL((dense_topk_partial_kernel<decltype(m)::value>), grid, dim3(DT_BLK), 0, s, q, Qn, g, G, (int)n, rows, (int)k,
                                   part);
                CH_LAUNCH_CHECK();
                return 0;
            }))
            return e;
    }
    hipLaunchKernelGGL(dense_topk_merge_kernel, dim3((unsigned)ceil_div64(Qn, 4)), dim3(256), 0, s, part, (int)nseg, Qn, (int)k, g_index_base,
                       out_idx, out_dist);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_dense_rerank(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, const int64_t *cand,
                               int32_t m, int32_t k, int64_t g_index_base, int64_t *out_idx, float *out_dist, void *stream) {
    if (int e = check_dense("dense_rerank", n, metric)) return e;
    CH_REQUIRE(m >= 1 && m <= RR_MAX && k >= 1 && k <= m, "dense_rerank: 1 <= k <= m <= 4096");
    CH_REQUIRE(Qn >= 0 && G >= 0, "dense_rerank: negative sizes");
    CH_REQUIRE(g_index_base >= 0 && g_index_base + G <= 0x100000000ll, "dense_rerank: keys hold 32-bit row indices (g_index_base + G <= 2^32)");
    if (Qn == 0) return 0;
    CH_REQUIRE(q && cand && out_idx && out_dist, "dense_rerank: null pointer");
    CH_REQUIRE(G == 0 || g != nullptr, "dense_rerank: null gallery");
    CH_REQUIRE(Qn <= 0x7FFFFFFFll, "dense_rerank: too many queries for one call");
    int P = 2;
    while (P < m) P <<= 1;
    const bool wide = n % 4 == 0 && ((uintptr_t)g & 15) == 0;
    const size_t lds = (size_t)P * sizeof(uint64_t) + 256 * sizeof(float) + (wide ? RR_BLK * RR_TS * sizeof(float) : 0);   // at most 51,200 bytes
    return dispatch_metric(metric, [&](auto mt) {
        constexpr int M = decltype(mt)::value;
        if (wide)
            hipLaunchKernelGGL((dense_rerank_kernel<M, true>), dim3((unsigned)Qn), dim3(RR_BLK), lds, (hipStream_t)stream, q, g, G, (int)n, cand,
                               (int)m, P, (int)k, g_index_base, out_idx, out_dist);
        else
            hipLaunchKernelGGL((dense_rerank_kernel<M, false>), dim3((unsigned)Qn), dim3(RR_BLK), lds, (hipStream_t)stream, q, g, G, (int)n, cand,
                               (int)m, P, (int)k, g_index_base, out_idx, out_dist);
        CH_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int ch_dense_rank_collect(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, const void *q_labels,
                                     const void *g_labels, int32_t LW, int64_t g_index_base, const int64_t *offsets, uint32_t *count,
                                     uint64_t *keys, void *stream) {
    return rank_collect_run("dense_rank_collect", DenseRanking{q, (int)n, (int)metric}, Qn, (const uint64_t *)g, G, q_labels, g_labels, (int)LW,
                            g_index_base, offsets, count, keys, (hipStream_t)stream);
}

extern "C" int ch_dense_rank_count(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, int64_t g_index_base,
                                   int32_t seg_rows, const int64_t *offsets, const uint64_t *keys, int32_t list_cap, uint32_t *bins,
                                   void *stream) {
    return rank_count_run("dense_rank_count", DenseRanking{q, (int)n, (int)metric}, Qn, (const uint64_t *)g, G, g_index_base, (int)seg_rows,
                          offsets, keys, (int)list_cap, bins, (hipStream_t)stream);
}
