// Reduction of real-valued codes (gfx950): the moments a PCA is fitted on and the projection that applies it (DESIGN.md section 2.0,
// "reduction").  Built with -ffp-contract=off: every multiply-add below is an fmaf that is written down.
//
// codes X [rows, n] fp32 row-major, 1 <= n <= 256; blocks of s = `block` columns (s divides n).  shift: fp32 [n] or NULL;
// y = fl32(x - shift), one rounding (y = x under NULL).  Block-diagonal matrices cross the ABI compact, as R does in itq.hip.
//
// Moments (pca_sum_kernel, pca_gram_kernel, pca_combine_kernel): one workgroup of 256 lanes per segment of seg_rows <= 4,096 rows.
//   sum[j]: P = max(1, 256 / n) lanes share column j; lane p adds rows p, p + P, p + 2 P, ... of the segment in this order (plain fp32
//   adds from 0.0f), then the P partials are added in the order p = 0 .. P - 1 -- a fixed two-level tree of at most seg_rows - 1 adds.
//   gram[b s + a, c]: the outputs a are taken in chunks of PC_JC = 16; a chunk walks the segment in tiles of T rows whose columns of the
//   chunk's block(s) are staged in LDS AS y (the subtraction is made once, at staging).  A lane owns the entries (j, c), c = lane / 16 +
//   16 k, of the chunk and walks the tile's rows in order, acc = fmaf(y_j, y_c, acc): ONE fp32 chain in row order of at most seg_rows
//   terms.  The product of an fmaf commutes, so entry (a, c) and entry (c, a) see the same chain: gram is exactly symmetric in a block.
//   A segment leaves its fp32 partials in the workspace; pca_combine_kernel adds them in segment order in fp64.  No atomics anywhere:
//   two runs give the same bits.
// Projection (pca_project_kernel): ONE function, pca_chain: for row i and output j of block b
//     acc = 0.0f;  for l = 0 .. s - 1 in this order:  acc = fmaf(fl32(x[i, b s + l] - shift[b s + l]), A_b[l, j], acc)
// A compact [n, t]: row b s + l holds A_b[l, :].  One lane per output, so a row projects to the same bits alone or in a batch; with
// t == s and no shift it is the chain of itq.hip's rotation.
#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"

namespace {

constexpr int PC_BLK = 256;
constexpr int PC_JC = 16;          // outputs of a chunk
constexpr int PC_MAX_N = 256;
constexpr int PC_MAX_SEG = 4096;   // rows of a segment: the longest fp32 chain
constexpr int PC_ACC = PC_MAX_N / PC_JC;   // entries of the Gram a lane owns at most (s = 256)
constexpr int PC_TILE_FLOATS = 4160;       // the largest T (n + 1) over n in [1, 256] (n = 64, T = 64)

// y = fl32(x - shift): one rounding, made where an operand is read
__device__ __forceinline__ float pca_y(float x, const float *shift, int col) { return shift ? x - shift[col] : x; }

// The chain of output j of block b for one row.  x: the row's entries of block b, consecutive; shift: NULL, or the block's entries of
// the shift; a: A_b[0, j], as floats between two rows of A_b.
__device__ __forceinline__ float pca_chain(const float *x, const float *shift, const float *a, int s, int as) {
    float acc = 0.0f;
#pragma unroll 4
    for (int l = 0; l < s; ++l) acc = fmaf(pca_y(x[l], shift, l), a[(size_t)l * as], acc);
    return acc;
}

// rows of a tile: about 4,096 entries of X, a multiple of 16 in [16, 64]
__host__ __device__ __forceinline__ int pca_tile_rows(int n) {
    const int t = 4096 / n / 16 * 16;
    return t < 16 ? 16 : t > 64 ? 64 : t;
}

__global__ __launch_bounds__(PC_BLK) void pca_sum_kernel(const float *__restrict__ X, int64_t rows, int n, const float *__restrict__ shift,
                                                         int seg_rows, float *__restrict__ part_sum) {
    __shared__ float part[PC_BLK];
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int64_t g0 = seg * seg_rows;
    const int nrows = (int)min((int64_t)seg_rows, rows - g0);
    const int P = PC_BLK / n < 1 ? 1 : PC_BLK / n;   // lanes of a column (n <= 256: P >= 1)
    const int p = tid / n, j = tid - p * n;
    float acc = 0.0f;
    if (p < P) {
        const float sh = shift ? shift[j] : 0.0f;
        const float *x = X + g0 * n + j;
        for (int r = p; r < nrows; r += P) {
            const float v = x[(size_t)r * n];
            acc += shift ? v - sh : v;
        }
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < n) {
        float t = part[tid];
        for (int q = 1; q < P; ++q) t += part[q * n + tid];
        part_sum[seg * n + tid] = t;
    }
}

template <int NK>
__global__ __launch_bounds__(PC_BLK) void pca_gram_kernel(const float *__restrict__ X, int64_t rows, int n, const float *__restrict__ shift,
                                                          int s, int seg_rows, float *__restrict__ part_gram) {
    __shared__ float Yt[PC_TILE_FLOATS];   // [T][stride]
    const int T = pca_tile_rows(n);
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int64_t g0 = seg * seg_rows;
    const int nrows = (int)min((int64_t)seg_rows, rows - g0);
    const float *Xseg = X + g0 * n;
    float *Gseg = part_gram + seg * (int64_t)n * s;
    const int jj = tid & (PC_JC - 1), sub = tid >> 4;   // the lane's output of a chunk; its first c
    for (int j0 = 0; j0 < n; j0 += PC_JC) {
        const int JC = min(PC_JC, n - j0);
        const int c0 = j0 / s * s, c1 = ((j0 + JC - 1) / s + 1) * s;   // the columns of X the chunk's blocks own (c1 <= n)
        const int Wc = c1 - c0, stride = Wc + 1;                       // T stride <= T (n + 1) <= PC_TILE_FLOATS
        const bool live = jj < JC;
        const int j = j0 + (live ? jj : 0);
        const int b = j / s, voff = b * s - c0;   // the lane's block, and where it starts inside a tile row
        float acc[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] = 0.0f;
        for (int t0 = 0; t0 < nrows; t0 += T) {   // the same trips for every lane: the barriers below are a workgroup's
            __syncthreads();   // the tile before is read
            for (int i = tid; i < T * Wc; i += PC_BLK) {
                const int r = i / Wc, c = i - r * Wc;
                Yt[r * stride + c] = t0 + r < nrows ? pca_y(Xseg[(size_t)(t0 + r) * n + c0 + c], shift, c0 + c) : 0.0f;
            }
            __syncthreads();
            if (live) {
                const int tr = min(T, nrows - t0);
#pragma unroll 8
                for (int r = 0; r < tr; ++r) {
                    const float ya = Yt[r * stride + (j - c0)];
                    const float *yr = Yt + r * stride + voff + sub;
#pragma unroll
                    for (int k = 0; k < NK; ++k)
                        if (sub + PC_JC * k < s) acc[k] = fmaf(ya, yr[PC_JC * k], acc[k]);
                }
            }
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (sub + PC_JC * k < s) Gseg[(size_t)j * s + sub + PC_JC * k] = acc[k];
        }
    }
}

// out[e] = the partials of entry e in segment order, in fp64: the n sums first, then (where asked for) the n s entries of the Gram
__global__ __launch_bounds__(PC_BLK) void pca_combine_kernel(const float *__restrict__ part_sum, const float *__restrict__ part_gram,
                                                             int64_t nseg, int n, int entries, double *__restrict__ out_sum,
                                                             double *__restrict__ out_gram) {
    const int e = blockIdx.x * PC_BLK + threadIdx.x;
    if (e < n) {
        double m = 0.0;
        for (int64_t sg = 0; sg < nseg; ++sg) m += (double)part_sum[sg * n + e];
        out_sum[e] = m;
    } else if (e - n < entries) {
        const int g = e - n;
        double m = 0.0;
        for (int64_t sg = 0; sg < nseg; ++sg) m += (double)part_gram[sg * entries + g];
        out_gram[g] = m;
    }
}

// one lane per output: the lanes of a wave read consecutive columns of A (and one or a few rows of X: broadcasts)
__global__ __launch_bounds__(PC_BLK) void pca_project_kernel(const float *__restrict__ X, int64_t rows, int n, const float *__restrict__ shift,
                                                             const float *__restrict__ A, int s, int t, float *__restrict__ out) {
    const int m = n / s * t;
    const int64_t o = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    if (o >= rows * m) return;
    const int64_t i = o / m;
    const int jo = (int)(o - i * m), b = jo / t, j = jo - b * t;
    out[o] = pca_chain(X + i * n + b * s, shift ? shift + b * s : nullptr, A + (size_t)b * s * t + j, s, t);
}

// Rows per segment where the caller leaves it open: about a thousand workgroups (four per CU) while a segment keeps at least 64
// rows, never more than 4,096; a multiple of 64 (the rule of the ITQ step).
int pca_seg_rows(int64_t rows) {
    return (int)std::max<int64_t>(64, std::min<int64_t>(PC_MAX_SEG, round_up64(ceil_div64(std::max<int64_t>(rows, 1), 1024), 64)));
}

int check_pca(const char *who, int64_t rows, int n, int block) {
    const std::string at = std::string(who) + ": ";
    CH_REQUIRE(n >= 1 && n <= PC_MAX_N, at + "n must be in [1, 256]");
    CH_REQUIRE(block >= 1 && n % block == 0, at + "block must be >= 1 and divide n");
    CH_REQUIRE(rows >= 0, at + "negative rows");
    return 0;
}

// f(std::integral_constant<int, NK>) for the smallest instance that holds ceil(s / 16) accumulators
template <class F>
int dispatch_pca_acc(int s, F &&f) {
    const int need = (s + PC_JC - 1) / PC_JC;
    if (need <= 1) return f(std::integral_constant<int, 1>{});
    if (need <= 2) return f(std::integral_constant<int, 2>{});
    if (need <= 4) return f(std::integral_constant<int, 4>{});
    if (need <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, PC_ACC>{});
}

}  // namespace

extern "C" size_t ch_pca_moments_workspace(int64_t rows, int32_t n, int32_t block, int32_t seg_rows, int32_t with_gram) {
    if (rows <= 0 || n < 1 || n > PC_MAX_N || block < 1 || n % block || seg_rows < 0 || seg_rows > PC_MAX_SEG) return 16;
    const int64_t nseg = ceil_div64(rows, seg_rows > 0 ? seg_rows : pca_seg_rows(rows));
    return (size_t)nseg * ((size_t)n + (with_gram ? (size_t)n * block : 0)) * sizeof(float) + 16;
}

extern "C" int ch_pca_moments(const float *codes, int64_t rows, int32_t n, int32_t block, const float *shift, int32_t seg_rows,
                              double *out_sum, double *out_gram, void *workspace, size_t workspace_bytes, void *stream) {
    if (int e = check_pca("pca_moments", rows, n, block)) return e;
    CH_REQUIRE(seg_rows >= 0 && seg_rows <= PC_MAX_SEG, "pca_moments: seg_rows must be in [0, 4096] (0: chosen here)");
    if (rows == 0) return 0;
    CH_REQUIRE(codes && out_sum, "pca_moments: null pointer");
    const int seg = seg_rows > 0 ? seg_rows : pca_seg_rows(rows);
    const int64_t nseg = ceil_div64(rows, seg);
    CH_REQUIRE(nseg <= 0x7FFFFFFFll, "pca_moments: too many segments for one call (raise seg_rows)");
    CH_REQUIRE(workspace && workspace_bytes >= ch_pca_moments_workspace(rows, n, block, seg_rows, out_gram != nullptr),
               "pca_moments: workspace too small");
    CH_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out_sum & 7) == 0 && ((uintptr_t)out_gram & 7) == 0,
               "pca_moments: workspace, out_sum and out_gram must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float *part_sum = (float *)workspace;
    float *part_gram = part_sum + nseg * n;
    hipLaunchKernelGGL(pca_sum_kernel, dim3((unsigned)nseg), dim3(PC_BLK), 0, st, codes, rows, (int)n, shift, seg, part_sum);
    CH_LAUNCH_CHECK();
    if (out_gram) {
        if (int e = dispatch_pca_acc(block, [&](auto nk) {
                constexpr int NK = decltype(nk)::value;
                hipLaunchKernelGGL((pca_gram_kernel<NK>), dim3((unsigned)nseg), dim3(PC_BLK), 0, st, codes, rows, (int)n, shift, (int)block, seg,
                                   part_gram);
                CH_LAUNCH_CHECK();
                return 0;
            }))
            return e;
    }
    const int entries = out_gram ? n * block : 0;
    hipLaunchKernelGGL(pca_combine_kernel, dim3((unsigned)ceil_div64(n + entries, PC_BLK)), dim3(PC_BLK), 0, st, part_sum, part_gram, nseg,
                       (int)n, entries, out_sum, out_gram);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_pca_project(const float *codes, int64_t rows, int32_t n, int32_t block, const float *shift, const float *A, int32_t t,
                              float *out, void *stream) {
    if (int e = check_pca("pca_project", rows, n, block)) return e;
    CH_REQUIRE(t >= 1 && t <= block, "pca_project: t must be in [1, block]");
    if (rows == 0) return 0;
    CH_REQUIRE(codes && A && out, "pca_project: null pointer");
    const int64_t outs = rows * (n / block * t);
    CH_REQUIRE(ceil_div64(outs, PC_BLK) <= 0x7FFFFFFFll, "pca_project: rows x bits too large for one call");
    hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)ceil_div64(outs, PC_BLK)), dim3(PC_BLK), 0, (hipStream_t)stream, codes, rows, (int)n,
                       shift, A, (int)block, (int)t, out);
    CH_LAUNCH_CHECK();
    return 0;
}
