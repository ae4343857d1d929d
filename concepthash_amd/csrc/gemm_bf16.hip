// bf16 MFMA GEMM with fused epilogues for the ConceptHash encoder (gfx950 / CDNA4).
//
//   C[m][n] = sum_k X[m][k] * W[n][k]        X: activations [M,K] bf16 row-major, W: nn.Linear weight [N,K] bf16
//
// This is the arithmetic of every Linear on the reference's hot path (HF CLIPAttention q/k/v/out_proj, CLIPMLP fc1/fc2,
// models/layers/adapter.py:46-60 down/up_proj, and the patch-embed Conv2d restated as im2col GEMM,
// models/arch/coop.py:452-466).  The reference runs them as fp32 torch ops; here operands are bf16, accumulation fp32.
//
// Structure (v1): 128x128x64 block tile, 4 waves (2x2), each wave a 64x64 sub-tile = 4x4 v_mfma_f32_16x16x32_bf16
// tiles.  Both operands are staged global->LDS with global_load_lds_dwordx4 (no VGPR round trip), double buffered,
// one barrier per K-step.  LDS rows are 128 B (64 bf16); the 16-B chunk index is XOR-swizzled with (row & 7), applied
// on the per-lane *source* address (the LDS-DMA destination is lane-linear) and again on the ds_read_b128 address,
// which makes every fragment read conflict free.
// The MFMA A operand is the WEIGHT tile and the B operand the ACTIVATION tile, so the accumulator holds D[n][m]:
// a lane owns 4 consecutive n for one m, i.e. 4 contiguous output elements -> 8-B bf16 / 16-B fp32 stores.
#include <cstdlib>

#include "ch_common.h"
#include "kernels.h"
#include "gemm_epilogue.h"
#include "gemm_tile.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int STAGE_BYTES = (BM + BN) * BK * 2;  // 32 KiB
constexpr int NTHREADS = 256;

// NT: the scale+residual epilogues' read-modify-write of the fp32 residual is non-temporal (gemm_epilogue.h: ld_resid).  A parameter of
// the KERNEL template on purpose: wrapping the body in an inlined function shared by two __global__ symbols changed the compiler's
// operand order of commutative instructions in every instance -- and one of the reordered forms is the packed-fp32 op_sel form
// that MI355X executes wrongly next to MFMA waves of another kernel.
template <int EPI, bool NT = false>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_bf16_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid & 1, wn = wid >> 1;

    const TileOrigin org = tile_origin<BM, BN>(p, blockIdx.x);
    const int m0 = org.m0, n0 = org.n0;

    // ---- staging addresses: the stage image is [X rows 0..127 ; W rows 0..127] x 128 B, 8 rows per wave-instruction.
    // wave w issues instructions i = 8w .. 8w+7; lane l -> row 8i + (l>>3), LDS chunk (l&7) holding source chunk
    // (l&7) ^ (row&7).
    const int lrow = lane >> 3;
    const int src_chunk = (lane & 7) ^ lrow;  // (8i + lrow) & 7 == lrow
    const char *gsrc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = (wid * 8 + j) * 8 + lrow;  // 0..255
        const bf16_t *base = row < BM ? p.X + (size_t)(m0 + row) * p.K : p.W + (size_t)(n0 + row - BM) * p.K;
        gsrc[j] = (const char *)(base + src_chunk * 8);
    }
    auto stage = [&](int buf, int kt) {
        char *dst = smem + buf * STAGE_BYTES + wid * 8 * 1024;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            __builtin_amdgcn_global_load_lds((gbl_void_t *)(gsrc[j] + (size_t)kt * BK * 2), (lds_void_t *)(dst + j * 1024),
                                             16, 0, 0);
    };

    f32x4 acc[4][4];
    zero_acc(acc);

    // fragment read offsets (bytes) inside a stage: row = sub*16 + (lane&15), chunk = (kk*4 + (lane>>4)) ^ (row&7)
    const int frow = lane & 15, fq = lane >> 4;
    const int nk = p.K / BK;

    f32x4 fold_v[5];
    if constexpr (ch_epi::traits<EPI>::fold) ch_epi::fold_stats_issue(p, m0, tid, fold_v);
    stage(0, 0);
    // read-modify-write epilogues: fetch the residual tile now, so that it arrives under the K loop
    constexpr bool PREF = ch_epi::traits<EPI>::scale_resid;
    ch_epi::ResidPrefetch rp;
    if constexpr (PREF) ch_epi::resid_prefetch<EPI, NT>(p, m0 + wm * 64, n0 + wn * 64, lane, rp);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (ch_epi::traits<EPI>::fold)  // per-row (mean, rstd) of the LN-folded input
        ch_epi::fold_stats_finish(p, tid, fold_v, (float *)(smem + 2 * STAGE_BYTES));
    __syncthreads();

    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
        const char *xs = smem + cur * STAGE_BYTES;
        const char *ws = xs + BM * BK * 2;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 wf[4], xf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int wr = wn * 64 + t * 16 + frow;
                wf[t] = *(const bf16x8 *)(ws + wr * 128 + (((kk * 4 + fq) ^ (wr & 7)) << 4));
                const int xr = wm * 64 + t * 16 + frow;
                xf[t] = *(const bf16x8 *)(xs + xr * 128 + (((kk * 4 + fq) ^ (xr & 7)) << 4));
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf[mt], acc[nt][mt], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue (gemm_epilogue.h): transpose through this wave's 16 KB of the idle staging LDS, full-line stores.
    // The loop's last __syncthreads() guarantees no wave still reads staged operands.
    ch_epi::store_tile<EPI, 4, PREF, NT>(p, acc, smem + wid * 16384, m0 + wm * 64, n0 + wn * 64, lane,
                                         (const float *)(smem + 2 * STAGE_BYTES) + 2 * (wm * 64), &rp);
}

template <int EPI>
int launch(const GemmParams &p0, hipStream_t s) {
    GemmParams p = p0;
    const dim3 grid(ch_gemm_plan_tiles(p, BM, BN));
    constexpr int lds = 2 * STAGE_BYTES + (ch_epi::is_fold(EPI) ? CH_FOLD_LDS_BYTES : 0);
    if constexpr (ch_epi::is_scale_resid(EPI)) {
        if (p.nt_resid) {
            if (int e = ch_gemm_launch<gemm_bf16_kernel<EPI, true>>(grid, NTHREADS, lds, s, p)) return e;
            ch_gemm_count_nt_launch(0);
            return 0;
        }
    }
    return ch_gemm_launch<gemm_bf16_kernel<EPI>>(grid, NTHREADS, lds, s, p);
}

}  // namespace

int ch_gemm_bf16_v1(const GemmParams &p, int epi, hipStream_t s) {
    if (int e = ch_gemm_check_common(p, epi)) return e;
    CH_REQUIRE(p.N % BN == 0, "gemm: N must be a multiple of 128");
    CH_REQUIRE(p.K % BK == 0, "gemm: K must be a multiple of 64");
    CH_REQUIRE(p.X_rows_alloc >= round_up64(p.M, BM), "gemm: X must be allocated for M rounded up to 128 rows");
    return ch_epi_dispatch(epi, [&](auto e) { return launch<e()>(p, s); });
}

// Estimated beyond-L2 read traffic for n-groups of gn tiles: every group re-streams X once; a group's weight panels are
// fetched once per XCD if they fit in half of the 4 MB L2, otherwise once per round of co-resident tiles.
int ch_gemm_group_n(int M, int N, int K, int bm, int bn, int forced) {
    const int tiles_n = N / bn, tiles_m = (M + bm - 1) / bm;
    const double xbytes = 2.0 * M * K, wpanel = 2.0 * bn * K, wbytes = 2.0 * N * K;
    const double rounds = (double)tiles_m * tiles_n / 256.0 + 1.0;
    if (forced > 0) return forced < tiles_n ? forced : tiles_n;   // model option "group_n" (tools/gemm_bench.py sweeps)
    int best = tiles_n;
    double best_cost = 1e300;
    for (int gn = 1; gn <= tiles_n; ++gn) {
        const int ng = (tiles_n + gn - 1) / gn;
        const bool fits = gn * wpanel <= 2.0e6;  // measured (fc1, K = 768): 4-5 panels (1.6-2.0 MB) 270 us, 6 panels (2.4 MB) 286 us
        const double cost = xbytes * ng + wbytes * 8.0 * (fits ? 1.0 : rounds);
        if (cost < best_cost - 1.0) {
            best_cost = cost;
            best = gn;
        }
    }
    return best;
}

// ---- dispatcher: the 256x256 ping-pong kernel when the shape allows it, this file's 128x128 kernel otherwise ---------
static std::atomic<int64_t> g_dispatch_count[5];   // 128x128 | 256x256 | non-temporal residual instance | non-temporal output instance | 256x384
void ch_gemm_count_nt_launch(int kind) { g_dispatch_count[2 + (kind != 0)].fetch_add(1, std::memory_order_relaxed); }
// residual tensors from this size up are streamed past the caches by the scale+residual epilogues (gemm_epilogue.h: ld_resid);
// the model option "resid_nt" (1 / -1) forces the choice
static int resid_nt_choice(const GemmParams &p, int epi) {
    if (!ch_epi::is_scale_resid(epi)) return 0;
    if (p.nt_resid_opt) return p.nt_resid_opt > 0;
    return std::max<int64_t>(p.M, p.footprint_rows) * p.N * 4 >= (48ll << 20);
}
// bf16 outputs of the plain / LN-folded epilogues from this size up (fc1's 316 MB and qkv's 237 MB at batch 256: read once, by the
// next kernel, out of HBM whatever the policy) are stored non-temporally by the 256x256 kernel, which leaves the caches to the
// operands: 12.15 -> 11.99 ms per encode step (profiles/r03_cache_policy_ab.txt).  The model option "nt_out" (1 / -1) forces the choice.
static int out_nt_choice(const GemmParams &p, int epi) {
    if (!ch_epi::may_nt_out(epi)) return 0;
    if (p.nt_out_opt) return p.nt_out_opt > 0;
    return std::max<int64_t>(p.M, p.footprint_rows) * p.N * 2 >= (128ll << 20);
}
// The one table from variant number to kernel (test taps, and the dispatcher when a caller forces a choice): the named launcher
// itself -- no cache-policy choice, no dispatcher argument checks, not counted.
int ch_gemm_launch_variant(int variant, const GemmParams &p, int epi, hipStream_t s) {
    switch (variant) {
        case 1: return ch_gemm_bf16_v1(p, epi, s);
        case 2: return ch_gemm_bf16_pp(p, epi, s);
        case 4:     // 256x256 kernel, coarse schedule
        case 8: {   // 256x256 kernel, free tail
            GemmParams q = p;
            q.pp_sched = variant == 4 ? 1 : 2;
            return ch_gemm_bf16_pp(q, epi, s);
        }
        case 3: return ch_gemm_bf16_dp(p, epi, s);
        case 5: return ch_gemm_bf16_ppp(p, epi, s);
        case 6: return ch_gemm_bf16_pq(p, epi, s);
        case 7: return ch_gemm_bf16_r4(p, epi, s);
        case 9: return ch_gemm_bf16_rows(p, epi, s);
        case 10: return ch_gemm_bf16_wide(p, epi, s);
    }
    if (variant >= 21 && variant <= 29) return ch_gemm_bf16_pp_dbg(p, variant - 20, s);    // timing-only / stamped builds
    if (variant >= 41 && variant <= 47) return ch_gemm_bf16_wide_dbg(p, variant - 40, s);  // timing-only builds of the 256x384 kernel
    ch_set_error("gemm: variant must be 1 .. 10, 21 .. 29 (256x256 timing builds) or 41 .. 47 (256x384 timing builds)");
    return 2;
}
// variant: 0 = the rule below; 7 = the rule with the ring kernel wherever it is supported; any other number = that kernel of
// ch_gemm_launch_variant after the cache-policy choice and the argument checks, not counted (test taps only: product callers pass nothing)
int ch_gemm_bf16(const GemmParams &p0, int epi, hipStream_t s, int variant) {
    GemmParams p = p0;
    p.nt_resid = resid_nt_choice(p, epi);
    p.nt_out = out_nt_choice(p, epi);
    if (ch_epi::is_dact(epi)) CH_REQUIRE(p.aux != nullptr, "gemm: derivative epilogue needs aux (the pre-activation)");
    if (ch_epi::is_act2(epi)) CH_REQUIRE(p.hb_out != nullptr, "gemm: two-output epilogue needs hb_out");
    if (ch_epi::is_fold(epi))
        CH_REQUIRE(p.stats_in && p.fold_c && p.K % 128 == 0 && p.K <= 1280 && p.ln_eps > 0.f,
                   "gemm: LN-folded epilogue needs stats_in, fold_c, ln_eps and K % 128 == 0, K <= 1280");
    if (ch_epi::is_stats(epi))
        CH_REQUIRE(p.stats_out && (!ch_epi::is_scale_resid(epi) || p.hb_out), "gemm: statistics epilogue needs stats_out (and hb_out)");
    if (variant != 0 && variant != 7) return ch_gemm_launch_variant(variant, p, epi, s);
    // Short-K GEMMs (the adapter up-projection, K = 384) are epilogue/HBM bound: two 128x128 workgroups per CU overlap one's
    // read-modify-write epilogue with the other's K loop and win there (measured: 152 -> 97 us per launch in the pipeline);
    // the 256x256 ping-pong kernel wins from K = 512 up.
    const int min_k = p.pp_min_k > 0 ? p.pp_min_k : 512;  // per model (option "pp_min_k"), not per process
    // Small grids: fewer than 128 tiles of 256x256 leave more than half of the 256 CUs idle; 128x128 tiles (4x as many, two
    // workgroups per CU) win there -- measured at 6,432 rows (batch 32): out 28 vs 36 us, fc2 57 vs 73 us; at 12,864 rows and
    // N = 768 (153 tiles) the two tie.  Not applied when CH_GEMM_PP_MIN_K pins the choice (parity tests on small fixtures).
    const int64_t tiles_pp = ceil_div64(p.M, 256) * (p.N / 256);
    const bool pp = ch_gemm_pp_supported(p) && p.K >= min_k && (p.pp_min_k > 0 || tiles_pp >= 128);
    // N = 384 (the adapter bottleneck of ViT-B/16) does not fit the 256x256 kernel; as 128x128 tiles it is LDS-port bound (64x64 wave
    // tiles).  experiments/gemm_wide.hip (256x384 tiles, 64x192 wave tiles, X read once, one round of the chip) is 9-14 % faster as an
    // isolated launch and neutral end to end (profiles/r04_gemm_wide_ab.txt): opt-in, model option "wide_kernel" = 1, experiments build.
    const bool wide = !pp && p.wide_opt > 0 && ch_gemm_wide_supported(p, epi);
    g_dispatch_count[pp ? 1 : wide ? 4 : 0].fetch_add(1, std::memory_order_relaxed);
    if (pp) return ch_gemm_bf16_pp(p, epi, s);
    if (wide) return ch_gemm_bf16_wide(p, epi, s);
    // N = 384 (the adapter bottleneck) as whole-row workgroups (experiments/gemm_rows.hip): one round of the chip instead of 2.36
    // rounds of 128x128 tiles, bit-identical -- and no faster (61 vs 59 us).  Opt-in: model option "gemm_rows", experiments build.
    if (p.rows_opt && p.small_kernel == 0 && p.M >= 128 * 128 && ch_gemm_rows_supported(p, epi)) return ch_gemm_bf16_rows(p, epi, s);
    // Small grids (batch <= 40 of ViT-B/16): every launch is one workgroup per CU walking a chain of L2 round trips; the four-stage ring
    // (gemm_r4.hip, bit-identical) keeps three K-steps in flight: -7 % per step at batch 8, -2.5 % at batch 32; slower at 51,456 rows.
    // (a non-temporal residual instance, chosen by size or forced by the option "resid_nt", exists in the two-phase kernel only and wins)
    const bool ring = (p.small_kernel == 2 || variant == 7 || (p.small_kernel == 0 && variant == 0 && p.M <= CH_RING_MAX_ROWS && !p.nt_resid)) &&
                      ch_gemm_r4_supported(p, epi);
    return ring ? ch_gemm_bf16_r4(p, epi, s) : ch_gemm_bf16_v1(p, epi, s);
}
// test tap: how many GEMMs the dispatcher has sent to the 128x128 (which = 0) / 256x256 ping-pong (which = 1) kernel, and how many
// launches ran the instance with the non-temporal residual read-modify-write (2) / the non-temporal bf16 output store (3); 4 = GEMMs sent
// to the 256x384 kernel
extern "C" int64_t ch_debug_gemm_dispatch_count(int32_t which) {
    return g_dispatch_count[which < 0 || which > 4 ? 0 : which].load(std::memory_order_relaxed);
}
