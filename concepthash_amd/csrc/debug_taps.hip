// Test / bench taps (include/concepthash_hip_debug.h): every ch_debug_* entry point that only wraps an internal launcher, on caller
// buffers.  Not on the product path: model.hip, train.hip and text_model.hip hold none.  Taps that read a file-local counter or
// flag stay next to it (gemm_bf16.hip, attention.hip, hamming.hip).
#include <algorithm>
#include <string>

#include "model_internal.h"
#include "../../include/concepthash_hip_debug.h"

// split-K workspace of the debug taps (off by default so that the 256x256 kernel stays bit-identical to the 128x128 one)
static bool g_debug_splitk = false;
static float *g_debug_ws = nullptr;
static unsigned *g_debug_cnt = nullptr;
// force: the call asks for the split itself (ch_debug_gemm_fwd); otherwise ch_debug_set_gemm_splitk decides
static int debug_attach_splitk(GemmParams &p, bool force = false) {
    if (!g_debug_splitk && !force) return 0;
    if (!g_debug_ws) {
        CH_CHECK_HIP(hipMalloc((void **)&g_debug_ws, CH_SPLITK_WS_BYTES));
        CH_CHECK_HIP(hipMalloc((void **)&g_debug_cnt, CH_SPLITK_CNT_BYTES));
        CH_CHECK_HIP(hipMemset(g_debug_cnt, 0, CH_SPLITK_CNT_BYTES));
    }
    p.splitk_ws = g_debug_ws;
    p.splitk_cnt = g_debug_cnt;
    p.force_split = 1;
    return 0;
}
extern "C" void ch_debug_set_gemm_splitk(int32_t on) { g_debug_splitk = on != 0; }

// ---- test / bench taps: one GEMM launch on caller buffers (tests/test_gemm_gpu.py, tools/gemm_bench.py) ----------------
// Each tap keeps its own argument checks, fills GemmParams through debug_gemm_params and ends in debug_gemm_launch.
static GemmParams debug_gemm_params(const void *X, int64_t X_rows_alloc, const void *W, const float *bias, int32_t M, int32_t N, int32_t K,
                                    void *out_bf16, int32_t ldo, const float *scale_ptr) {
    GemmParams p{};
    p.X = (const bf16_t *)X; p.W = (const bf16_t *)W; p.M = M; p.N = N; p.K = K; p.X_rows_alloc = X_rows_alloc;
    p.bias = bias; p.out_bf16 = (bf16_t *)out_bf16; p.ldo = ldo; p.scale_ptr = scale_ptr;
    return p;
}
// direct: the kernel that `variant` names, by itself (ch_gemm_launch_variant: no cache-policy choice, no dispatcher checks, not
// counted); otherwise the dispatcher, which runs its rule (variant 0) or that kernel after its own choices and checks
static int debug_gemm_launch(GemmParams &p, int epi, void *stream, int variant, bool direct, bool splitk) {
    if (splitk)
        if (int e = debug_attach_splitk(p)) return e;
    return direct ? ch_gemm_launch_variant(variant, p, epi, (hipStream_t)stream) : ch_gemm_bf16(p, epi, (hipStream_t)stream, variant);
}
extern "C" int ch_debug_gemm(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias,
                             int32_t M, int32_t N, int32_t K, int32_t epi, void *out_bf16, int32_t ldo, float *resid,
                             int32_t ldr, const float *scale_ptr, const void *addend, void *stream) {
    CH_REQUIRE(X && W, "debug_gemm: null operand");
    CH_REQUIRE(epi >= EPI_BIAS && epi <= EPI_SCALE_RESID, "debug_gemm: epilogue must be one of the non-patch modes");
    GemmParams p = debug_gemm_params(X, X_rows_alloc, W, bias, M, N, K, out_bf16, ldo, scale_ptr);
    p.resid = resid; p.ldr = ldr; p.addend = (const bf16_t *)addend; p.ld_addend = N;
    // every kernel and timing-only build by number; any other number is the dispatcher's rule
    const bool direct = (variant >= 1 && variant <= 10) || (variant >= 21 && variant <= 29) || (variant >= 41 && variant <= 47);
    return debug_gemm_launch(p, epi, stream, direct ? variant : 0, direct, true);
}
extern "C" int ch_debug_gemm_ln(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias,
                                int32_t M, int32_t N, int32_t K, int32_t epi, void *out_bf16, int32_t ldo, float *resid,
                                int32_t ldr, const float *scale_ptr, const void *addend, const float *stats_in,
                                const float *fold_c, float ln_eps, float *stats_out, void *hb_out, void *stream) {
    CH_REQUIRE(X && W, "debug_gemm_ln: null operand");
    CH_REQUIRE(epi >= EPI_BIAS_STATS && epi <= EPI_FOLD_GELU, "debug_gemm_ln: epilogue must be one of the LayerNorm-fold modes");
    GemmParams p = debug_gemm_params(X, X_rows_alloc, W, bias, M, N, K, out_bf16, ldo, scale_ptr);
    p.resid = resid; p.ldr = ldr; p.addend = (const bf16_t *)addend; p.ld_addend = N;
    p.stats_in = stats_in; p.fold_c = fold_c; p.ln_eps = ln_eps; p.stats_out = stats_out; p.hb_out = (bf16_t *)hb_out; p.ld_hb = N;
    // 5, 6, 7 by themselves; 1, 2, 4, 8, 9, 10 through the dispatcher (cache policy by size, its checks); anything else is the rule
    const bool direct = variant >= 5 && variant <= 7;
    const bool forced = variant == 1 || variant == 2 || variant == 4 || variant == 8 || variant == 9 || variant == 10;
    return debug_gemm_launch(p, epi, stream, direct || forced ? variant : 0, direct, true);
}
// variant of the two taps below: 0 = dispatcher, 1 = 128x128 two-phase, 2 / 4 = 256x256 ping-pong (fine / coarse schedule), 7 = ring
// direct: a named kernel by itself (the training and patch taps); false: the same kernel through the dispatcher (ch_debug_gemm_fwd)
static int debug_gemm_launch_checked(GemmParams &p, int epi, void *stream, int variant, const char *what, bool direct = true) {
    if (variant != 0 && variant != 1 && variant != 2 && variant != 4 && variant != 7) {
        ch_set_error(std::string(what) + ": variant must be 0 (dispatcher), 1, 2, 4 or 7");
        return 2;
    }
    return debug_gemm_launch(p, epi, stream, variant, direct && variant != 0, false);
}
// The training-step epilogues (kernels.h): 11 / 12 = (*scale_ptr, 12 only) * bf16(acc + bias) * act'(aux), aux [M, ldo] bf16 in the layout
// of out_bf16; 13 / 14 = out_bf16 = the LN-folded linear (stats_in, fold_c, ln_eps as ch_debug_gemm_ln), hb_out [M, ld_hb] = act(out_bf16).
extern "C" int ch_debug_gemm_train(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias, int32_t M,
                                   int32_t N, int32_t K, int32_t epi, void *out_bf16, int32_t ldo, const void *aux, const float *scale_ptr,
                                   const float *stats_in, const float *fold_c, float ln_eps, void *hb_out, int32_t ld_hb, void *stream) {
    CH_REQUIRE(X && W && bias && out_bf16, "debug_gemm_train: null operand");
    CH_REQUIRE(epi >= EPI_BIAS_DACT_QUICK && epi <= EPI_FOLD_ACT2_GELU, "debug_gemm_train: epilogue must be one of the training modes (11 .. 14)");
    CH_REQUIRE(M > 0 && N > 0 && K > 0, "debug_gemm_train: empty problem");
    CH_REQUIRE(ldo >= N && ldo % 8 == 0, "debug_gemm_train: ldo must be >= N and a multiple of 8 (16-byte row chunks)");
    const bool dact = epi == EPI_BIAS_DACT_QUICK || epi == EPI_BIAS_DACT_GELU;
    if (dact) {
        CH_REQUIRE(aux != nullptr, "debug_gemm_train: the derivative epilogues need aux");
        // a workgroup reads the aux rows of its tile while other workgroups store theirs: in place is not what the training step does
        const char *a0 = (const char *)aux, *o0 = (const char *)out_bf16;
        const size_t span = ((size_t)(M - 1) * ldo + N) * sizeof(bf16_t);
        CH_REQUIRE(a0 + span <= o0 || o0 + span <= a0, "debug_gemm_train: aux and out_bf16 must not overlap");
    } else {
        CH_REQUIRE(hb_out != nullptr && stats_in && fold_c, "debug_gemm_train: the two-output epilogues need hb_out, stats_in and fold_c");
        CH_REQUIRE(ld_hb >= N && ld_hb % 8 == 0, "debug_gemm_train: ld_hb must be >= N and a multiple of 8 (16-byte row chunks)");
        CH_REQUIRE(K % 128 == 0 && K <= 1280 && ln_eps > 0.f, "debug_gemm_train: LN-folded epilogue needs K % 128 == 0, K <= 1280, ln_eps > 0");
        CH_REQUIRE(hb_out != out_bf16, "debug_gemm_train: hb_out and out_bf16 must be distinct");
    }
    GemmParams p = debug_gemm_params(X, X_rows_alloc, W, bias, M, N, K, out_bf16, ldo, scale_ptr);
    p.aux = (const bf16_t *)aux;
    p.stats_in = stats_in; p.fold_c = fold_c; p.ln_eps = ln_eps; p.hb_out = (bf16_t *)hb_out; p.ld_hb = ld_hb;
    return debug_gemm_launch_checked(p, epi, stream, variant, "debug_gemm_train");
}
// The ten forward epilogues (0 .. 4, 6 .. 10) with every leading dimension and launch option of GemmParams the product sets, always
// THROUGH the dispatcher: variant 0 is its rule, 1 / 2 / 4 / 7 that kernel after the dispatcher's cache-policy choice and checks (so the
// non-temporal instances are reachable and counted).  The alignment each leading dimension needs is the widest access of store_tile /
// resid_prefetch to that tensor: 16-byte stores of out_bf16 (8-byte ones in EPI_BIAS_RESID), 16-byte loads / stores of resid, 8-byte loads
// of addend and 8-byte stores of hb_out.
extern "C" int ch_debug_gemm_fwd(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias, int32_t M, int32_t N,
                                 int32_t K, int32_t epi, void *out_bf16, int32_t ldo, float *resid, int32_t ldr, const float *scale_ptr,
                                 const void *addend, int32_t ld_addend, const float *stats_in, const float *fold_c, float ln_eps,
                                 float *stats_out, void *hb_out, int32_t ld_hb, int32_t nt_resid_opt, int32_t nt_out_opt, int32_t group_n_opt,
                                 int32_t rev, int32_t splitk, void *stream) {
    CH_REQUIRE(X && W && bias, "debug_gemm_fwd: null operand");
    CH_REQUIRE((epi >= EPI_BIAS && epi <= EPI_SCALE_RESID) || (epi >= EPI_BIAS_STATS && epi <= EPI_FOLD_GELU),
               "debug_gemm_fwd: epilogue must be one of the forward modes (0 .. 4, 6 .. 10)");
    CH_REQUIRE(M > 0 && N > 0 && K > 0, "debug_gemm_fwd: empty problem");
    CH_REQUIRE(nt_resid_opt >= -1 && nt_resid_opt <= 1 && nt_out_opt >= -1 && nt_out_opt <= 1 && group_n_opt >= 0 && (rev == 0 || rev == 1) &&
               (splitk == 0 || splitk == 1), "debug_gemm_fwd: nt_*_opt must be -1, 0 or 1, group_n_opt >= 0, rev and splitk 0 or 1");
    const bool scale_resid = epi == EPI_SCALE_RESID || epi == EPI_SCALE_RESID_STATS;
    const bool fold = epi >= EPI_FOLD_BIAS && epi <= EPI_FOLD_GELU;
    if (!scale_resid) {
        CH_REQUIRE(out_bf16 != nullptr, "debug_gemm_fwd: this epilogue writes out_bf16");
        if (epi == EPI_BIAS_RESID)
            CH_REQUIRE(ldo >= N && ldo % 4 == 0, "debug_gemm_fwd: ldo must be >= N and a multiple of 4 (8-byte stores of the bf16 copy)");
        else
            CH_REQUIRE(ldo >= N && ldo % 8 == 0, "debug_gemm_fwd: ldo must be >= N and a multiple of 8 (16-byte row chunks)");
    }
    if (epi == EPI_BIAS_RESID || scale_resid) {
        CH_REQUIRE(resid != nullptr, "debug_gemm_fwd: the residual epilogues need resid");
        CH_REQUIRE(ldr >= N && ldr % 4 == 0, "debug_gemm_fwd: ldr must be >= N and a multiple of 4 (16-byte row chunks)");
    }
    if (epi == EPI_BIAS_RESID) CH_REQUIRE((const void *)resid != (const void *)out_bf16, "debug_gemm_fwd: resid and out_bf16 must be distinct");
    if (scale_resid) {
        CH_REQUIRE(scale_ptr != nullptr, "debug_gemm_fwd: the scale + residual epilogues need scale_ptr");
        if (addend) CH_REQUIRE(ld_addend >= N && ld_addend % 4 == 0, "debug_gemm_fwd: ld_addend must be >= N and a multiple of 4 (8-byte loads)");
    }
    if (epi == EPI_BIAS_STATS || epi == EPI_SCALE_RESID_STATS) CH_REQUIRE(stats_out != nullptr, "debug_gemm_fwd: the statistics epilogues need stats_out");
    if (epi == EPI_SCALE_RESID_STATS) {
        CH_REQUIRE(hb_out != nullptr, "debug_gemm_fwd: epilogue 7 needs hb_out");
        CH_REQUIRE(ld_hb >= N && ld_hb % 4 == 0, "debug_gemm_fwd: ld_hb must be >= N and a multiple of 4 (8-byte stores)");
        CH_REQUIRE((const void *)hb_out != (const void *)resid, "debug_gemm_fwd: hb_out and resid must be distinct");
    }
    if (fold)
        CH_REQUIRE(stats_in && fold_c && K % 128 == 0 && K <= 1280 && ln_eps > 0.f,
                   "debug_gemm_fwd: LN-folded epilogue needs stats_in, fold_c, K % 128 == 0, K <= 1280, ln_eps > 0");
    CH_REQUIRE(!splitk || variant == 2, "debug_gemm_fwd: the split-K tail belongs to the 256x256 kernel (variant 2)");
    GemmParams p = debug_gemm_params(X, X_rows_alloc, W, bias, M, N, K, out_bf16, ldo, scale_ptr);
    p.resid = resid; p.ldr = ldr; p.addend = (const bf16_t *)addend; p.ld_addend = ld_addend;
    p.stats_in = stats_in; p.fold_c = fold_c; p.ln_eps = ln_eps; p.stats_out = stats_out; p.hb_out = (bf16_t *)hb_out; p.ld_hb = ld_hb;
    p.nt_resid_opt = nt_resid_opt; p.nt_out_opt = nt_out_opt; p.group_n_opt = group_n_opt; p.rev = rev;
    if (variant == 7) {
        // the dispatcher takes 7 as "the ring wherever it is supported" and would fall back to its rule: here 7 means the ring or an error
        CH_REQUIRE(ch_gemm_r4_supported(p, epi), "debug_gemm_fwd: the ring kernel needs N % 128 == 0, K % 32 == 0, K >= 96, X padded to 128 rows");
        CH_REQUIRE(((int64_t)M + 255) / 256 * (N / 256) < 128, "debug_gemm_fwd: at this size the dispatcher's rule takes the 256x256 kernel, not the ring");
    }
    if (splitk)
        if (int e = debug_attach_splitk(p, true)) return e;
    return debug_gemm_launch_checked(p, epi, stream, variant, "debug_gemm_fwd", false);
}
// The patch-embedding epilogue: resid[(img * tokens_per_img + 1 + patch) * ldr + n] = acc + pos[(1 + patch) * N + n] for row
// m = img * patches_per_img + patch of X W^T (no bias); every other row of resid is left alone.
extern "C" int ch_debug_gemm_patch(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, int32_t M, int32_t N, int32_t K,
                                   float *resid, int32_t ldr, const float *pos, int32_t tokens_per_img, int32_t patches_per_img,
                                   void *stream) {
    CH_REQUIRE(X && W && resid && pos, "debug_gemm_patch: null operand");
    CH_REQUIRE(M > 0 && N > 0 && K > 0, "debug_gemm_patch: empty problem");
    CH_REQUIRE(ldr >= N && ldr % 4 == 0, "debug_gemm_patch: ldr must be >= N and a multiple of 4 (16-byte row chunks)");
    CH_REQUIRE(patches_per_img >= 1 && tokens_per_img >= 1 + patches_per_img, "debug_gemm_patch: tokens_per_img must be >= 1 + patches_per_img");
    CH_REQUIRE(M % patches_per_img == 0, "debug_gemm_patch: M must be a whole number of images");
    GemmParams p = debug_gemm_params(X, X_rows_alloc, W, nullptr, M, N, K, nullptr, 0, nullptr);
    p.resid = resid; p.ldr = ldr; p.pos = pos; p.tokens_per_img = tokens_per_img; p.patches_per_img = patches_per_img;
    return debug_gemm_launch_checked(p, EPI_PATCH, stream, variant, "debug_gemm_patch");
}
extern "C" int32_t ch_debug_experiments_built(void) {
#ifdef CH_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

extern "C" int ch_debug_attention(const void *qkv, int32_t B, int32_t ntok, int32_t heads, void *out, void *stream) {
    CH_REQUIRE(qkv && out, "debug_attention: null pointer");
    return ch_attention((const bf16_t *)qkv, B, ntok, heads, (bf16_t *)out, (hipStream_t)stream);
}
extern "C" int ch_debug_attention_ex(const void *qkv, int32_t B, int32_t ntok, int32_t heads, void *out, float *cattn, int32_t ncon,
                                     int32_t compact, int32_t kernel, void *stream) {
    CH_REQUIRE(qkv && out, "debug_attention_ex: null pointer");
    return ch_attention((const bf16_t *)qkv, B, ntok, heads, (bf16_t *)out, (hipStream_t)stream, cattn, ncon, compact != 0, false, kernel);
}

extern "C" int ch_debug_attention_causal(const void *qkv, int32_t B, int32_t ntok, int32_t heads, void *out, void *stream) {
    CH_REQUIRE(qkv && out, "debug_attention_causal: null pointer");
    return ch_attention_causal((const bf16_t *)qkv, B, ntok, heads, (bf16_t *)out, (hipStream_t)stream);
}

// ---- the text tower's own two kernels (text_model.hip), each launcher by itself on caller buffers (tests/test_text_chain_gpu.py).
// Device pointers only: ids and eos are NOT range-checked here (ch_text_encode checks its host arrays; the test supplies valid ones).
extern "C" int ch_debug_text_embed(const int32_t *ids, int32_t rows, int32_t T, int32_t D, const float *tok, const float *pos, float *H,
                                   void *stream) {
    CH_REQUIRE(ids && tok && pos && H, "debug_text_embed: null argument");
    return ch_text_embed(ids, rows, T, D, tok, pos, H, (hipStream_t)stream);
}
extern "C" int ch_debug_text_pool(const float *H, const int32_t *eos, int32_t nrows, int32_t T, int32_t D, const float *w, const float *b,
                                  float eps, float *out, void *stream) {
    CH_REQUIRE(H && w && b && out, "debug_text_pool: null argument");
    return ch_text_pool(H, eos, nrows, T, D, w, b, eps, out, (hipStream_t)stream);
}

extern "C" int ch_debug_adapter(const void *A, float *H, int32_t M, int32_t D, int32_t b, const float *Wd, const float *bd,
                                const float *gamma, const float *beta, const void *Wu_bf16_padded, const float *bu,
                                const float *scale, void *work_wdf, float *work_c, float *work_d, int32_t dbg, void *stream) {
    // Wd [b, D] fp32, Wu [D, bpad] bf16 (already padded); work_*: caller scratch for the folded weights ([bpad, D] bf16, [bpad] x2)
    const int bpad = (int)round_up64(b, 128);
    hipStream_t s = (hipStream_t)stream;
    if (int e = ch_fold_ln(Wd, bd, gamma, beta, b, bpad, D, (bf16_t *)work_wdf, work_c, work_d, s)) return e;
    AdapterParams p{};
    p.A = (const bf16_t *)A; p.H = H; p.M = M; p.D = D; p.bpad = bpad; p.Wd = (const bf16_t *)work_wdf; p.c = work_c; p.d = work_d;
    p.Wu = (const bf16_t *)Wu_bf16_padded; p.bu = bu; p.scale = scale; p.eps = 1e-5f; p.dbg = dbg;
    return ch_adapter_fused(p, s);
}

// test tap: copy the first nbytes of one workspace buffer (as the last ch_encode / ch_encode_hidden left it) to `out`
extern "C" int ch_debug_copy_buffer(ch_model *m, int32_t which, void *out, int64_t nbytes, void *stream) {
    CH_REQUIRE(m != nullptr && out != nullptr && nbytes >= 0, "debug_copy_buffer: null pointer");
    const int64_t rows = m->rows_alloc, D = m->cfg.dim;
    const void *src = nullptr;
    int64_t size = 0;
    switch (which) {
        case 0: src = m->H; size = rows * D * 4; break;
        case 1: src = m->Xn; size = rows * D * 2; break;
        case 2: src = m->QKV; size = rows * 3 * D * 2; break;
        case 3: src = m->AO; size = rows * D * 2; break;
        case 4: src = m->A; size = rows * D * 2; break;
        case 5: src = m->AD; size = rows * std::max(m->bpad, 128) * 2; break;
        case 6: src = m->F1; size = rows * (int64_t)m->cfg.ffn * 2; break;
        default: CH_REQUIRE(false, "debug_copy_buffer: which must be 0..6 (H, Xn, QKV, AO, A, AD, F1)");
    }
    CH_REQUIRE(nbytes <= size, "debug_copy_buffer: more bytes requested than the buffer holds");
    CH_CHECK_HIP(hipMemcpyAsync(out, src, (size_t)nbytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// test tap: the centre arrays of a handle (`center` as ingested, and what ch_model_create folded from it)
extern "C" int ch_debug_model_centers(ch_model *m, int32_t which, float *out, void *stream) {
    CH_REQUIRE(m != nullptr && out != nullptr, "debug_model_centers: null pointer");
    CH_REQUIRE(which >= 0 && which <= 2, "debug_model_centers: which must be 0 (center), 1 (center_l2) or 2 (center_bin)");
    const float *src = which == 0 ? m->center : which == 1 ? m->center_l2 : m->center_bin;
    const size_t cols = which == 0 ? m->cfg.center_dim : m->cfg.nbit;
    CH_CHECK_HIP(hipMemcpyAsync(out, src, sizeof(float) * (size_t)m->cfg.nclass * cols, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---- kernel taps of the training step ----------------------------------------------------------------------------------------
extern "C" int ch_debug_attention_bwd(const void *qkv, const void *dO, int32_t B, int32_t ntok, int32_t heads, void *dqkv, const float *dpext,
                                      int32_t ncon, void *stream) {
    CH_REQUIRE(qkv && dO && dqkv, "debug_attention_bwd: null argument");
    return ch_attention_bwd((const bf16_t *)qkv, (const bf16_t *)dO, B, ntok, heads, (bf16_t *)dqkv, (hipStream_t)stream, dpext, ncon);
}
extern "C" int ch_debug_attention_bwd_ex(const void *qkv, const void *dO, int32_t B, int32_t ntok, int32_t heads, void *dqkv, const float *dpext,
                                         int32_t ncon, int32_t kernel, void *stream) {
    CH_REQUIRE(qkv && dO && dqkv, "debug_attention_bwd_ex: null argument");
    return ch_attention_bwd((const bf16_t *)qkv, (const bf16_t *)dO, B, ntok, heads, (bf16_t *)dqkv, (hipStream_t)stream, dpext, ncon, kernel);
}
extern "C" int ch_debug_wgrad(const void *A, int32_t lda, const void *Bm, int32_t ldb, int64_t rows, int64_t rows_alloc, int32_t N,
                              int32_t K, float *out, void *stream) {
    CH_REQUIRE(A && Bm && out, "debug_wgrad: null argument");
    ChDeviceTemp ws;
    if (ws.get(sizeof(float) * ch_wgrad_ws_floats(rows, N, K))) return 1;
    const int e = ch_wgrad_tn((bf16_t *)A, lda, (const bf16_t *)Bm, ldb, rows, rows_alloc, N, K, out, ws.as<float>(), (hipStream_t)stream);
    (void)hipStreamSynchronize((hipStream_t)stream);
    return e;
}
// row statistics of x are computed here (hb_stats on an fp32 copy is what the chain does; the tap takes bf16 x and derives the
// partials from it through an fp32 round trip), then ln_bwd; xhat_out (optional) is ln_bwd's own by-product store of x_hat, as the
// training step takes it (normalize has a tap of its own, ch_debug_normalize_bf16)
extern "C" int ch_debug_ln_bwd(const void *dyg, const void *x, int64_t rows, int32_t D, float eps, const float *dres_in, float *dres_out,
                               void *out_b, void *xhat_out, void *stream) {
    CH_REQUIRE(dyg && x && dres_in, "debug_ln_bwd: null argument");
    hipStream_t s = (hipStream_t)stream;
    ChDeviceTemp tst, txf, thb;
    if (tst.get(sizeof(float) * rows * (D / 64) * 2) || txf.get(sizeof(float) * rows * D) || thb.get(sizeof(bf16_t) * rows * D)) return 1;
    float *st = tst.as<float>(), *xf = txf.as<float>();
    bf16_t *hb = thb.as<bf16_t>();
    int e = 0;
    {   // bf16 -> fp32 (exact) by a strided 2-byte copy into the high halves
        CH_CHECK_HIP(hipMemsetAsync(xf, 0, sizeof(float) * rows * D, s));
        CH_CHECK_HIP(hipMemcpy2DAsync((char *)xf + 2, 4, x, 2, 2, (size_t)rows * D, hipMemcpyDeviceToDevice, s));
    }
    e = ch_hb_stats(xf, rows, D, hb, st, s);
    if (!e) e = ch_ln_bwd((const bf16_t *)dyg, (const bf16_t *)x, st, rows, D, eps, dres_in, dres_out, (bf16_t *)out_b, s, (bf16_t *)xhat_out);
    (void)hipStreamSynchronize(s);
    return e;
}
extern "C" int ch_debug_act(const void *g, const void *pre, int64_t n, int32_t act, const float *scale_ptr, int32_t backward, void *out,
                            void *stream) {
    CH_REQUIRE(pre && out, "debug_act: null argument");
    if (backward) return ch_act_bwd((const bf16_t *)g, (const bf16_t *)pre, n, act, scale_ptr, (bf16_t *)out, (hipStream_t)stream);
    return ch_act_fwd((const bf16_t *)pre, n, act, (bf16_t *)out, (hipStream_t)stream);
}

// ---- the training step's row, reduction and gradient-assembly launchers, each by itself (tests/test_train_rowkernels_gpu.py) ------
// One launcher per tap, on caller buffers; a tap allocates only the workspace its launcher asks for and waits for the stream
// before that workspace is released.
extern "C" int ch_debug_hb_stats(const float *H, int64_t rows, int32_t D, void *hb, float *stats, void *stream) {
    CH_REQUIRE(H && hb && stats && rows > 0, "debug_hb_stats: null argument");
    return ch_hb_stats(H, rows, D, (bf16_t *)hb, stats, (hipStream_t)stream);
}
extern "C" int ch_debug_normalize_bf16(const void *x, const float *stats, int64_t rows, int32_t D, float eps, void *out, void *stream) {
    CH_REQUIRE(x && stats && out && rows > 0, "debug_normalize_bf16: null argument");
    return ch_normalize_bf16((const bf16_t *)x, stats, rows, D, eps, (bf16_t *)out, (hipStream_t)stream);
}
extern "C" int ch_debug_colsum(const void *A, int32_t is_f32, int32_t lda, int64_t rows, int32_t N, float *out, void *stream) {
    CH_REQUIRE(A && out && rows > 0 && N > 0 && lda >= N, "debug_colsum: null argument or empty problem");
    ChDeviceTemp ws;
    if (ws.get(sizeof(float) * ch_colsum_ws_floats(N))) return 1;
    const int e = ch_colsum(A, is_f32, lda, rows, N, out, ws.as<float>(), (hipStream_t)stream);
    (void)hipStreamSynchronize((hipStream_t)stream);
    return e;
}
// job j: out[j][0 .. 4 * n4[j]) = sum over c < nchunks[j] of partial[j][c][.]; the four arrays are host arrays of njobs entries
extern "C" int ch_debug_reduce_partials_multi(int32_t njobs, const float *const *partial, float *const *out, const int32_t *nchunks,
                                              const int32_t *n4, void *stream) {
    CH_REQUIRE(njobs >= 1 && njobs <= 4 && partial && out && nchunks && n4, "debug_reduce_partials_multi: 1..4 jobs, no null array");
    ChReduceJob jobs[4];
    for (int j = 0; j < njobs; ++j) {
        CH_REQUIRE(partial[j] && out[j] && nchunks[j] >= 1 && n4[j] >= 1, "debug_reduce_partials_multi: empty job");
        jobs[j] = ChReduceJob{partial[j], out[j], nchunks[j], n4[j]};
    }
    return ch_reduce_partials_multi(jobs, njobs, (hipStream_t)stream);
}
extern "C" int ch_debug_transpose_f32_to_bf16(const float *src, int32_t R, int32_t C, int32_t ld_src, const float *colscale, void *dst,
                                              int32_t ld_dst, void *stream) {
    CH_REQUIRE(src && dst && R > 0 && C > 0 && ld_src >= C && ld_dst >= R, "debug_transpose_f32_to_bf16: null argument or short leading dimension");
    return ch_transpose_f32_to_bf16(src, R, C, ld_src, colscale, (bf16_t *)dst, ld_dst, (hipStream_t)stream);
}
extern "C" int ch_debug_transpose_bf16(const void *src, int32_t R, int32_t C, int32_t ld_src, void *dst, int32_t ld_dst, void *stream) {
    CH_REQUIRE(src && dst && R > 0 && C > 0 && ld_src >= C && ld_dst >= R, "debug_transpose_bf16: null argument or short leading dimension");
    return ch_transpose_bf16((const bf16_t *)src, R, C, ld_src, (bf16_t *)dst, ld_dst, (hipStream_t)stream);
}
extern "C" int ch_debug_adapter_refresh(const float *params, int64_t stride, int32_t nad, int32_t D, int32_t b, int32_t bpad, void *down_wf,
                                        float *fold_c, float *fold_d, void *up_w, void *up_wT, void *down_wgT, void *stream) {
    CH_REQUIRE(params && down_wf && fold_c && fold_d && up_w && up_wT && down_wgT, "debug_adapter_refresh: null argument");
    CH_REQUIRE(nad >= 1 && D > 0 && b > 0 && bpad >= b, "debug_adapter_refresh: empty problem or bpad < b");
    return ch_adapter_refresh(params, stride, nad, D, b, bpad, (bf16_t *)down_wf, fold_c, fold_d, (bf16_t *)up_w, (bf16_t *)up_wT,
                              (bf16_t *)down_wgT, (hipStream_t)stream);
}
extern "C" int ch_debug_adapter_grads(const float *G, const float *cu, const float *T, const float *cd, const float *params, int32_t D, int32_t b,
                                      int32_t bpad, float *grads, int32_t nad, int64_t stride, void *stream) {
    CH_REQUIRE(G && cu && T && cd && params && grads, "debug_adapter_grads: null argument");
    CH_REQUIRE(nad >= 1 && D > 0 && b > 0 && bpad >= b, "debug_adapter_grads: empty problem or bpad < b");
    ChDeviceTemp ws;
    if (ws.get(sizeof(float) * ch_adapter_grads_ws_floats(nad))) return 1;
    const int e = ch_adapter_grads(G, cu, T, cd, params, D, b, bpad, grads, ws.as<float>(), (hipStream_t)stream, nad, stride);
    (void)hipStreamSynchronize((hipStream_t)stream);
    return e;
}
// W / dW / db: host arrays of nparts device pointers (the row blocks' own allocations)
extern "C" int ch_debug_fold_grads(const float *T, const float *c, const float *gamma, const float *beta, int32_t D, int32_t nparts,
                                   int32_t rows_each, const float *const *W, float *const *dW, float *const *db, float *dgamma, float *dbeta,
                                   void *stream) {
    CH_REQUIRE(T && c && gamma && beta && W && dW && db && dgamma && dbeta, "debug_fold_grads: null argument");
    CH_REQUIRE(nparts >= 1 && nparts <= 3 && rows_each >= 1, "debug_fold_grads: 1..3 row blocks of at least one row");
    ChFoldGradParts parts{};
    parts.nparts = nparts;
    parts.rows_each = rows_each;
    for (int p = 0; p < nparts; ++p) {
        CH_REQUIRE(W[p] && dW[p] && db[p], "debug_fold_grads: null row block");
        parts.W[p] = W[p];
        parts.dW[p] = dW[p];
        parts.db[p] = db[p];
    }
    return ch_fold_grads(T, c, gamma, beta, D, parts, dgamma, dbeta, (hipStream_t)stream);
}
extern "C" int ch_debug_embed_bwd(float *X, float *dY, int32_t B, int32_t ntok, int32_t np, int32_t D, const float *cls_pos0, const float *ctx,
                                  const float *gamma, float eps, void *dx_patch, void *stream) {
    CH_REQUIRE(X && dY && cls_pos0 && ctx && gamma && dx_patch, "debug_embed_bwd: null argument");
    CH_REQUIRE(B >= 1 && np >= 1 && ntok > 1 + np, "debug_embed_bwd: ntok must be 1 + np + the number of concept rows (>= 1)");
    return ch_embed_bwd(X, dY, B, ntok, np, D, cls_pos0, ctx, gamma, eps, (bf16_t *)dx_patch, (hipStream_t)stream);
}
extern "C" int ch_debug_small_ln_bwd(const float *dy, const float *x, const float *gamma, int32_t rows, int32_t D, float eps, float *dx,
                                     void *stream) {
    CH_REQUIRE(dy && x && gamma && dx && rows >= 1 && D >= 1, "debug_small_ln_bwd: null argument or empty problem");
    return ch_small_ln_bwd(dy, x, gamma, rows, D, eps, dx, (hipStream_t)stream);
}
extern "C" int ch_debug_token_rows_sum(const float *dX, int32_t B, int32_t ntok, int32_t nrows, int32_t D, float *out, void *stream) {
    CH_REQUIRE(dX && out && B >= 1 && nrows >= 1 && nrows <= ntok && D >= 1, "debug_token_rows_sum: null argument or nrows outside 1..ntok");
    return ch_token_rows_sum(dX, B, ntok, nrows, D, out, (hipStream_t)stream);
}
extern "C" int ch_debug_concept_rows_sum(const float *dH, int32_t B, int32_t ntok, int32_t Q, int32_t D, float *out, void *stream) {
    CH_REQUIRE(dH && out && B >= 1 && Q >= 1 && Q <= ntok && D >= 1, "debug_concept_rows_sum: null argument or Q outside 1..ntok");
    return ch_concept_rows_sum(dH, B, ntok, Q, D, out, (hipStream_t)stream);
}
extern "C" int ch_debug_scatter_concept_rows(const float *dhf, int32_t B, int32_t ntok, int32_t Q, int32_t D, float *dH, void *dHb, void *stream) {
    CH_REQUIRE(dhf && dH && dHb && B >= 1 && Q >= 1 && Q <= ntok && D >= 1, "debug_scatter_concept_rows: null argument or Q outside 1..ntok");
    return ch_scatter_concept_rows(dhf, B, ntok, Q, D, dH, (bf16_t *)dHb, (hipStream_t)stream);
}
extern "C" int ch_debug_expand_head_rows(const void *src, int32_t is_f32, int32_t B, int32_t ntok, int32_t Q, int32_t D, void *dst, void *stream) {
    CH_REQUIRE(src && dst && B >= 1 && Q >= 1 && Q < ntok && D >= 1, "debug_expand_head_rows: null argument or Q outside 1..ntok-1");
    return ch_expand_head_rows(src, is_f32, B, ntok, Q, D, dst, (hipStream_t)stream);
}
extern "C" int ch_debug_gather_concept_rows(const float *H, int32_t B, int32_t ntok, int32_t Q, int32_t D, float *out, void *stream) {
    CH_REQUIRE(H && out && B >= 1 && Q >= 1 && Q <= ntok && D >= 1, "debug_gather_concept_rows: null argument or Q outside 1..ntok");
    return ch_gather_concept_rows(H, B, ntok, Q, D, out, (hipStream_t)stream);
}

// ---- the forward row kernels (rowops.hip), the hashing head (head.hip) and the load-time folds (small_f32.hip), each launcher by
// itself on caller buffers (tests/test_forward_kernels_gpu.py)
extern "C" int ch_debug_im2col(const void *images, int32_t image_dtype, int32_t B, int32_t image, int32_t patch, int32_t Kp, void *out,
                               void *stream) {
    CH_REQUIRE(images && out && (image_dtype == 0 || image_dtype == 1), "debug_im2col: null argument or image_dtype not 0 (fp32) / 1 (bf16)");
    CH_REQUIRE(B >= 1 && patch >= 1 && image >= patch && image % patch == 0, "debug_im2col: the image must be a whole number of patches");
    return ch_im2col(images, image_dtype, B, image, patch, Kp, (bf16_t *)out, (hipStream_t)stream);
}
extern "C" int ch_debug_assemble_preln(float *H, int32_t B, int32_t ntok, int32_t np, int32_t D, const float *cls_pos0, const float *ctx,
                                       const float *pre_w, const float *pre_b, const float *ln_w, const float *ln_b, float eps, void *xn,
                                       void *stream) {
    CH_REQUIRE(H && cls_pos0 && ctx && pre_w && pre_b && ln_w && ln_b && xn, "debug_assemble_preln: null argument");
    CH_REQUIRE(B >= 1 && np >= 1 && ntok > 1 + np, "debug_assemble_preln: ntok must be 1 + np + the number of concept rows (>= 1)");
    return ch_assemble_preln(H, B, ntok, np, D, cls_pos0, ctx, pre_w, pre_b, ln_w, ln_b, eps, (bf16_t *)xn, (hipStream_t)stream);
}
extern "C" int ch_debug_layernorm_f32(const float *x, int64_t rows, int32_t D, const float *w, const float *b, float eps, void *out,
                                      void *stream) {
    CH_REQUIRE(x && w && b && out && rows > 0, "debug_layernorm_f32: null argument");
    return ch_layernorm_f32(x, rows, D, w, b, eps, (bf16_t *)out, (hipStream_t)stream);
}
extern "C" int ch_debug_layernorm_bf16(const void *x, int64_t rows, int32_t D, const float *w, const float *b, float eps, void *out,
                                       int32_t kernel, void *stream) {
    CH_REQUIRE(x && w && b && out && rows > 0, "debug_layernorm_bf16: null argument");
    return ch_layernorm_bf16((const bf16_t *)x, rows, D, w, b, eps, (bf16_t *)out, (hipStream_t)stream, kernel);
}
extern "C" int ch_debug_gather_head_rows(const float *H, int32_t B, int32_t ntok, int32_t ncon, int32_t D, float *out, void *stream) {
    CH_REQUIRE(H && out && D >= 4, "debug_gather_head_rows: null argument");
    return ch_gather_head_rows(H, B, ntok, ncon, D, out, (hipStream_t)stream);
}
// Every HeadParams pointer goes through as given, nulls included: an optional output is asked for by passing its buffer.  The operands
// that an output reads must come with it (the kernel would read them), and the two workspaces are allocated here.
extern "C" int ch_debug_head(const float *H, int32_t B, int32_t ntok, int32_t D, int32_t Q, int32_t nbit, int32_t C, int32_t P,
                             const float *hash_pe, const float *hash_fc, const float *bn_scale, const float *bn_shift,
                             const float *center_l2, const float *center_bin, const float *concept_pe, const float *concept_cent_l2,
                             const float *post_w, const float *post_b, const float *vis_proj, float ln_eps, float *out_codes,
                             void *out_packed, float *out_logits_cont, float *out_logits_bin, float *out_logits_concept,
                             float *out_hash_features, float *out_image_features, void *stream) {
    CH_REQUIRE(H && hash_pe && hash_fc && bn_scale && bn_shift && out_codes, "debug_head: null argument");
    CH_REQUIRE(B >= 1 && D >= 1 && Q >= 1 && nbit >= 1 && ntok > Q, "debug_head: empty problem or ntok <= Q");
    CH_REQUIRE(!(out_logits_cont || out_logits_bin) || (center_l2 && center_bin && C >= 1), "debug_head: the code logits need both centre arrays");
    CH_REQUIRE(!out_logits_concept || (concept_pe && concept_cent_l2 && C >= 1), "debug_head: the concept logits need concept_pe and the centroids");
    CH_REQUIRE(!out_image_features || (post_w && post_b && vis_proj && P >= 1), "debug_head: the image features need post_w, post_b and vis_proj");
    hipStream_t s = (hipStream_t)stream;
    ChDeviceTemp txn, tcls;
    if (out_logits_concept && txn.get(sizeof(float) * (size_t)B * Q * D)) return 1;
    if (out_image_features && tcls.get(sizeof(float) * (size_t)B * D)) return 1;
    HeadParams p{};
    p.H = H; p.B = B; p.ntok = ntok; p.D = D; p.Q = Q; p.nbit = nbit; p.C = C; p.P = P;
    p.hash_pe = hash_pe; p.hash_fc = hash_fc; p.bn_scale = bn_scale; p.bn_shift = bn_shift;
    p.center_l2 = center_l2; p.center_bin = center_bin; p.concept_pe = concept_pe; p.concept_cent_l2 = concept_cent_l2;
    p.post_w = post_w; p.post_b = post_b; p.vis_proj = vis_proj; p.ln_eps = ln_eps;
    p.out_codes = out_codes; p.out_packed = (uint64_t *)out_packed; p.out_logits_cont = out_logits_cont; p.out_logits_bin = out_logits_bin;
    p.out_logits_concept = out_logits_concept; p.out_hash_features = out_hash_features; p.out_image_features = out_image_features;
    p.ws_xn = txn.as<float>(); p.ws_cls = tcls.as<float>();
    const int e = ch_head(p, s);
    (void)hipStreamSynchronize(s);
    return e;
}
extern "C" int ch_debug_small_linear(const float *x, int32_t rows, int32_t in_f, const float *W, const float *b, int32_t out_f, int32_t act,
                                     float *y, void *stream) {
    CH_REQUIRE(x && W && y && rows >= 1 && in_f >= 1 && out_f >= 1, "debug_small_linear: null argument or empty problem");
    return ch_small_linear(x, rows, in_f, W, b, out_f, act, y, (hipStream_t)stream);
}
extern "C" int ch_debug_small_layernorm(const float *x, int32_t rows, int32_t D, const float *w, const float *b, float eps, float *y,
                                        void *stream) {
    CH_REQUIRE(x && w && b && y && rows >= 1 && D >= 1, "debug_small_layernorm: null argument or empty problem");
    return ch_small_layernorm(x, rows, D, w, b, eps, y, (hipStream_t)stream);
}
extern "C" int ch_debug_small_add(const float *a, const float *b, int64_t n, float *y, void *stream) {
    CH_REQUIRE(a && b && y && n >= 1, "debug_small_add: null argument or empty problem");
    return ch_small_add(a, b, n, y, (hipStream_t)stream);
}
extern "C" int ch_debug_small_mha(const float *qkv, int32_t T, int32_t P, int32_t heads, float *out, void *stream) {
    CH_REQUIRE(qkv && out && T >= 1 && heads >= 1 && P >= heads, "debug_small_mha: null argument or empty problem");
    return ch_small_mha(qkv, T, P, heads, out, (hipStream_t)stream);
}
extern "C" int ch_debug_small_l2norm(const float *x, int32_t rows, int32_t cols, float *out_l2, float *out_bin, void *stream) {
    CH_REQUIRE(x && out_l2 && rows >= 1 && cols >= 1, "debug_small_l2norm: null argument or empty problem");
    return ch_small_l2norm(x, rows, cols, out_l2, out_bin, (hipStream_t)stream);
}
extern "C" int ch_debug_convert_bf16(const float *x, int64_t rows, int32_t cols, int32_t cols_pad, void *out, void *stream) {
    CH_REQUIRE(x && out && rows >= 1 && cols >= 1 && cols_pad >= cols, "debug_convert_bf16: null argument or cols_pad < cols");
    return ch_convert_bf16(x, rows, cols, cols_pad, (bf16_t *)out, (hipStream_t)stream);
}
extern "C" int ch_debug_bn_fold(const float *w, const float *b, const float *mean, const float *var, int32_t n, float eps, float *scale,
                                float *shift, void *stream) {
    CH_REQUIRE(w && b && mean && var && scale && shift && n >= 1, "debug_bn_fold: null argument or empty problem");
    return ch_bn_fold(w, b, mean, var, n, eps, scale, shift, (hipStream_t)stream);
}
extern "C" int ch_debug_fold_ln(const float *Wd, const float *bd, const float *gamma, const float *beta, int32_t b, int32_t bpad, int32_t D,
                                void *Wdf, float *c, float *d, void *stream) {
    CH_REQUIRE(Wd && bd && gamma && beta && Wdf && c && d, "debug_fold_ln: null argument");
    CH_REQUIRE(b >= 1 && bpad >= b && D >= 1, "debug_fold_ln: empty problem or bpad < b");
    return ch_fold_ln(Wd, bd, gamma, beta, b, bpad, D, (bf16_t *)Wdf, c, d, (hipStream_t)stream);
}
