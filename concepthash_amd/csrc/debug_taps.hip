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
static int debug_attach_splitk(GemmParams &p) {
    if (!g_debug_splitk) return 0;
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
static int debug_gemm_launch_checked(GemmParams &p, int epi, void *stream, int variant, const char *what) {
    if (variant != 0 && variant != 1 && variant != 2 && variant != 4 && variant != 7) {
        ch_set_error(std::string(what) + ": variant must be 0 (dispatcher), 1, 2, 4 or 7");
        return 2;
    }
    return debug_gemm_launch(p, epi, stream, variant, variant != 0, false);
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
// partials from it through an fp32 round trip), then ln_bwd; xhat_out (optional) receives normalize(x)
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
    if (!e) e = ch_ln_bwd((const bf16_t *)dyg, (const bf16_t *)x, st, rows, D, eps, dres_in, dres_out, (bf16_t *)out_b, s);
    if (!e && xhat_out) e = ch_normalize_bf16((const bf16_t *)x, st, rows, D, eps, (bf16_t *)xhat_out, s);
    (void)hipStreamSynchronize(s);
    return e;
}
extern "C" int ch_debug_act(const void *g, const void *pre, int64_t n, int32_t act, const float *scale_ptr, int32_t backward, void *out,
                            void *stream) {
    CH_REQUIRE(pre && out, "debug_act: null argument");
    if (backward) return ch_act_bwd((const bf16_t *)g, (const bf16_t *)pre, n, act, scale_ptr, (bf16_t *)out, (hipStream_t)stream);
    return ch_act_fwd((const bf16_t *)pre, n, act, (bf16_t *)out, (hipStream_t)stream);
}
