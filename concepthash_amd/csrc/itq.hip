// Learned code rotation (gfx950): one ITQ step and the rotation itself ("learned rotation").  Built with
// -ffp-contract=off: every multiply-add below is an fmaf that is written down.
//
// codes V [rows, n] fp32 row-major, 1 <= n <= 256.  R is block-diagonal with blocks of s = `block` columns (s divides n) and crosses the
// ABI compact, [n, s] fp32 row-major: row b s + l holds R_b[l, :].
//
// The rotation is ONE function, itq_chain: for row i and output j of block b = j / s
//     acc = 0.0f;  for l = 0 .. s - 1 in this order:  acc = fmaf(V[i, b s + l], R_b[l, j - b s], acc)
// Both kernels call it -- the step on operands staged in LDS, the rotate kernel on the ones in memory -- so a row rotates to the same
// bits alone or in a batch, in the fit or in the apply.  Sign: B = z > 0 ? +1 : -1 (pack_sign's rule: an exact zero is a 0 bit).
//
// The step (itq_step_kernel): one workgroup per segment of seg_rows <= 4,096 rows, 256 lanes.  The outputs j are taken in chunks of
// IT_JC = 16; a chunk walks the segment in tiles of T rows.  Per tile: the columns of V the chunk's blocks own go into LDS (each tile
// element is read from memory once per chunk whose block owns it: once where s <= 16 divides 16, s / 16 times otherwise -- the
// repeats of a segment, at most 4 MB, come out of the L2 / Infinity Cache); a lane owns output j of up to four rows (row, row + 16, ...) and forms their z by the chain, leaves B in
// LDS, and the 16 lanes of a row add |z| and z^2 by a fixed butterfly into the row's two fp32 sums (LDS, chunk after chunk in order);
// then a lane owns the entries M[j, l], l = lane / 16 + 16 k, of the chunk and walks the tile's rows in order,
// acc = fmaf(B[i, j], V[i, b s + l], acc) -- B is +-1, so that is acc +- V rounded once: an fp32 chain of at most seg_rows terms.
// A segment leaves its n x s fp32 partial of M and its two fp64 sums (rows in a fixed lane order, a fixed tree over the lanes) in
// the workspace; itq_combine_kernel adds the partials in segment order in fp64.  No atomics anywhere: two runs give the same bits.
#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"

namespace {

constexpr int IT_BLK = 256;
constexpr int IT_JC = 16;          // outputs of a chunk
constexpr int IT_MAX_N = 256;
constexpr int IT_MAX_SEG = 4096;   // rows of a segment: the longest fp32 chain of M
constexpr int IT_ACC = IT_MAX_N / IT_JC;   // entries of M a lane owns at most (s = 256); a kernel instance holds NK >= ceil(s / 16) of them

// The chain of output j for np <= P rows at once (each row's chain is its own; the rows share the loads of R and hide each other's
// latency).  v: the first row's entries of block b, consecutive, vs floats to the next row of the lane; r: R_b[0, j - b s], rs floats
// between two rows of R_b as r sees them.
template <int P>
__device__ __forceinline__ void itq_chain(const float *v, int vs, int np, const float *r, int s, int rs, float (&z)[P]) {
#pragma unroll
    for (int p = 0; p < P; ++p) z[p] = 0.0f;
#pragma unroll 4
    for (int l = 0; l < s; ++l) {
        const float rl = r[(size_t)l * rs];
#pragma unroll
        for (int p = 0; p < P; ++p)
            if (p < np) z[p] = fmaf(v[(size_t)p * vs + l], rl, z[p]);
    }
}

// rows of a tile: about 4,096 entries of V, a multiple of 16 in [16, 64]
__host__ __device__ __forceinline__ int itq_tile_rows(int n) {
    const int t = 4096 / n / 16 * 16;
    return t < 16 ? 16 : t > 64 ? 64 : t;
}

// LDS of a step workgroup, in floats: row sums [2][seg_rows], V tile [T][n + 1], R chunk [s][16], B tile [T][16]; behind them the
// 2 x 256 doubles of the closing tree
__host__ __device__ __forceinline__ size_t itq_lds_floats(int n, int s, int seg_rows) {
    const int T = itq_tile_rows(n);
    return (size_t)2 * seg_rows + (size_t)T * (n + 1) + (size_t)s * IT_JC + (size_t)T * IT_JC;
}

template <int NK>
__global__ __launch_bounds__(IT_BLK) void itq_step_kernel(const float *__restrict__ V, int64_t rows, int n, const float *__restrict__ R,
                                                          int s, int seg_rows, float *__restrict__ part_M, double *__restrict__ part_stats) {
    extern __shared__ __align__(16) double it_lds[];
    const int T = itq_tile_rows(n);
    double *red = it_lds;                         // [2][256]
    float *rowsum = (float *)(it_lds + 2 * IT_BLK);   // [2][seg_rows]: |z|, z^2
    float *Vt = rowsum + 2 * (size_t)seg_rows;    // [T][stride]
    float *Rc = Vt + (size_t)T * (n + 1);         // [s][16]
    float *Bt = Rc + (size_t)s * IT_JC;           // [T][16]
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int64_t g0 = seg * seg_rows;
    const int nrows = (int)min((int64_t)seg_rows, rows - g0);
    const float *Vseg = V + g0 * n;
    float *Mseg = part_M + seg * (int64_t)n * s;
    for (int r = tid; r < nrows; r += IT_BLK) {
        rowsum[r] = 0.0f;
        rowsum[seg_rows + r] = 0.0f;
    }
    const int jj = tid & (IT_JC - 1), sub = tid >> 4;   // the lane's output of a chunk; its row of a pass / its first l
    for (int j0 = 0; j0 < n; j0 += IT_JC) {
        const int JC = min(IT_JC, n - j0);
        const int c0 = j0 / s * s, c1 = ((j0 + JC - 1) / s + 1) * s;   // the columns of V the chunk's blocks own
        const int Wc = c1 - c0, stride = Wc + 1;
        const bool live = jj < JC;
        const int j = j0 + (live ? jj : 0);
        const int b = j / s, voff = b * s - c0;   // the lane's block, and where it starts inside a tile row
        __syncthreads();   // the chunk before has read Rc
        for (int i = tid; i < s * IT_JC; i += IT_BLK) {
            const int l = i >> 4, c = i & (IT_JC - 1);
            float v = 0.0f;
            if (c < JC) {
                const int jc = j0 + c, bc = jc / s;
                v = R[((size_t)bc * s + l) * s + (jc - bc * s)];
            }
            Rc[i] = v;
        }
        float acc[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] = 0.0f;
        for (int t0 = 0; t0 < nrows; t0 += T) {   // the same trips for every lane: the barriers below are a workgroup's
            __syncthreads();   // the tile before is read, Rc is written
            for (int i = tid; i < T * Wc; i += IT_BLK) {
                const int r = i / Wc, c = i - r * Wc;
                Vt[r * stride + c] = t0 + r < nrows ? Vseg[(size_t)(t0 + r) * n + c0 + c] : 0.0f;
            }
            __syncthreads();
            float zs[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // rows sub, sub + 16, ... of the tile (T <= 64); rows past the segment's end are zeros in the tile
            if (live) itq_chain<4>(Vt + sub * stride + voff, (IT_BLK / IT_JC) * stride, T / (IT_BLK / IT_JC), Rc + jj, s, IT_JC, zs);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int r = sub + p * (IT_BLK / IT_JC);
                if (r >= T) break;   // the same for every lane
                const bool valid = live && t0 + r < nrows;
                const float z = zs[p];
                Bt[r * IT_JC + jj] = valid ? (z > 0.0f ? 1.0f : -1.0f) : 0.0f;
                float a1 = valid ? fabsf(z) : 0.0f, a2 = valid ? z * z : 0.0f;
#pragma unroll
                for (int o = IT_JC / 2; o > 0; o >>= 1) {   // the 16 lanes of a row: a fixed butterfly
                    a1 += __shfl_xor(a1, o, 64);
                    a2 += __shfl_xor(a2, o, 64);
                }
                if (jj == 0 && t0 + r < nrows) {
                    rowsum[t0 + r] += a1;
                    rowsum[seg_rows + t0 + r] += a2;
                }
            }
            __syncthreads();
            if (live) {
                const int tr = min(T, nrows - t0);
#pragma unroll 8
                for (int r = 0; r < tr; ++r) {
                    const float bv = Bt[r * IT_JC + jj];
                    const float *vr = Vt + r * stride + voff + sub;
#pragma unroll
                    for (int k = 0; k < NK; ++k)
                        if (sub + IT_JC * k < s) acc[k] = fmaf(bv, vr[IT_JC * k], acc[k]);
                }
            }
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (sub + IT_JC * k < s) Mseg[(size_t)j * s + sub + IT_JC * k] = acc[k];
        }
    }
    __syncthreads();
    // the segment's sums: a lane takes rows tid, tid + 256, ... in order, then a fixed tree over the lanes
    double l1 = 0.0, cs = 0.0;
    for (int r = tid; r < nrows; r += IT_BLK) {
        const double a1 = (double)rowsum[r], a2 = (double)rowsum[seg_rows + r];
        l1 += a1;
        if (a2 > 0.0) cs += a1 / sqrt((double)n * a2);   // a zero row: cosine 0
    }
    red[tid] = l1;
    red[IT_BLK + tid] = cs;
    __syncthreads();
    for (int o = IT_BLK / 2; o > 0; o >>= 1) {
        if (tid < o) {
            red[tid] += red[tid + o];
            red[IT_BLK + tid] += red[IT_BLK + tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part_stats[2 * seg] = red[0];
        part_stats[2 * seg + 1] = red[IT_BLK];
    }
}

// out_M[e] = the partials of entry e in segment order, in fp64; the first lane of the grid does the same for the two sums
__global__ __launch_bounds__(IT_BLK) void itq_combine_kernel(const float *__restrict__ part_M, const double *__restrict__ part_stats,
                                                             int64_t nseg, int entries, double *__restrict__ out_M,
                                                             double *__restrict__ out_stats) {
    const int e = blockIdx.x * IT_BLK + threadIdx.x;
    if (e < entries) {
        double m = 0.0;
        for (int64_t sg = 0; sg < nseg; ++sg) m += (double)part_M[sg * entries + e];
        out_M[e] = m;
    }
    if (e == 0) {
        double l1 = 0.0, cs = 0.0;
        for (int64_t sg = 0; sg < nseg; ++sg) {
            l1 += part_stats[2 * sg];
            cs += part_stats[2 * sg + 1];
        }
        out_stats[0] = l1;
        out_stats[1] = cs;
    }
}

// one lane per output: the 64 lanes of a wave read consecutive columns of R (and one or a few rows of V: broadcasts)
__global__ __launch_bounds__(IT_BLK) void itq_rotate_kernel(const float *__restrict__ V, int64_t rows, int n, const float *__restrict__ R,
                                                            int s, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * IT_BLK + threadIdx.x;
    if (t >= rows * n) return;
    const int64_t i = t / n;
    const int j = (int)(t - i * n), b = j / s;
    float z[1];
    itq_chain<1>(V + i * n + b * s, 0, 1, R + (size_t)b * s * s + (j - b * s), s, s, z);
    out[t] = z[0];
}

// Rows per segment where the caller leaves it open: about a thousand workgroups (four per CU) while a segment keeps at least 64
// rows, never more than 4,096; a multiple of 64.
int itq_seg_rows(int64_t rows) {
    return (int)std::max<int64_t>(64, std::min<int64_t>(IT_MAX_SEG, round_up64(ceil_div64(std::max<int64_t>(rows, 1), 1024), 64)));
}

int check_itq(const char *who, int64_t rows, int n, int block) {
    const std::string at = std::string(who) + ": ";
    CH_REQUIRE(n >= 1 && n <= IT_MAX_N, at + "n must be in [1, 256]");
    CH_REQUIRE(block >= 1 && n % block == 0, at + "block must be >= 1 and divide n");
    CH_REQUIRE(rows >= 0, at + "negative rows");
    return 0;
}

// f(std::integral_constant<int, NK>) for the smallest instance that holds ceil(s / 16) accumulators
template <class F>
int dispatch_itq_acc(int s, F &&f) {
    const int need = (s + IT_JC - 1) / IT_JC;
    if (need <= 1) return f(std::integral_constant<int, 1>{});
    if (need <= 2) return f(std::integral_constant<int, 2>{});
    if (need <= 4) return f(std::integral_constant<int, 4>{});
    if (need <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, IT_ACC>{});
}

template <int NK>
struct itq_lds_once {
    static ch_once_per_device once;
};
template <int NK>
ch_once_per_device itq_lds_once<NK>::once;

}  // namespace

extern "C" size_t ch_itq_step_workspace(int64_t rows, int32_t n, int32_t block, int32_t seg_rows) {
    if (rows <= 0 || n < 1 || n > IT_MAX_N || block < 1 || n % block || seg_rows < 0 || seg_rows > IT_MAX_SEG) return 16;
    const int64_t nseg = ceil_div64(rows, seg_rows > 0 ? seg_rows : itq_seg_rows(rows));
    return (size_t)nseg * (2 * sizeof(double) + (size_t)n * block * sizeof(float)) + 16;
}

extern "C" int ch_itq_step(const float *codes, int64_t rows, int32_t n, const float *R, int32_t block, int32_t seg_rows, double *out_M,
                           double *out_stats, void *workspace, size_t workspace_bytes, void *stream) {
    if (int e = check_itq("itq_step", rows, n, block)) return e;
    CH_REQUIRE(seg_rows >= 0 && seg_rows <= IT_MAX_SEG, "itq_step: seg_rows must be in [0, 4096] (0: chosen here)");
    if (rows == 0) return 0;
    CH_REQUIRE(codes && R && out_M && out_stats, "itq_step: null pointer");
    const int seg = seg_rows > 0 ? seg_rows : itq_seg_rows(rows);
    const int64_t nseg = ceil_div64(rows, seg);
    CH_REQUIRE(nseg <= 0x7FFFFFFFll, "itq_step: too many segments for one call (raise seg_rows)");
    CH_REQUIRE(workspace && workspace_bytes >= ch_itq_step_workspace(rows, n, block, seg_rows), "itq_step: workspace too small");
    CH_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out_M & 7) == 0 && ((uintptr_t)out_stats & 7) == 0,
               "itq_step: workspace, out_M and out_stats must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double *part_stats = (double *)workspace;
    float *part_M = (float *)(part_stats + 2 * nseg);
    const size_t lds = 2 * IT_BLK * sizeof(double) + itq_lds_floats(n, block, seg) * sizeof(float);   // at most 76 KB
    if (int e = dispatch_itq_acc(block, [&](auto nk) {
            constexpr int NK = decltype(nk)::value;
            if (int e2 = ch_func_max_lds((const void *)itq_step_kernel<NK>, 80 * 1024, itq_lds_once<NK>::once)) return e2;
            hipLaunchKernelGGL((itq_step_kernel<NK>), dim3((unsigned)nseg), dim3(IT_BLK), lds, st, codes, rows, (int)n, R, (int)block, seg,
                               part_M, part_stats);
            CH_LAUNCH_CHECK();
            return 0;
        }))
        return e;
    const int entries = n * block;
    hipLaunchKernelGGL(itq_combine_kernel, dim3((unsigned)ceil_div64(entries, IT_BLK)), dim3(IT_BLK), 0, st, part_M, part_stats, nseg, entries,
                       out_M, out_stats);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_itq_rotate(const float *codes, int64_t rows, int32_t n, const float *R, int32_t block, float *out, void *stream) {
    if (int e = check_itq("itq_rotate", rows, n, block)) return e;
    if (rows == 0) return 0;
    CH_REQUIRE(codes && R && out, "itq_rotate: null pointer");
    CH_REQUIRE(ceil_div64(rows * n, IT_BLK) <= 0x7FFFFFFFll, "itq_rotate: rows x n too large for one call");
    hipLaunchKernelGGL(itq_rotate_kernel, dim3((unsigned)ceil_div64(rows * n, IT_BLK)), dim3(IT_BLK), 0, (hipStream_t)stream, codes, rows,
                       (int)n, R, (int)block, out);
    CH_LAUNCH_CHECK();
    return 0;
}
