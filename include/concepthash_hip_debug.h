/*
 * concepthash_hip_debug.h -- test / bench taps of libconcepthash_hip.so (MI355X / gfx950).
 *
 * NOT part of the drop-in boundary (include/concepthash_hip.h): single-kernel launches on caller buffers with the kernel
 * chosen per call, and workspace copies that tests/ and tools/ use to pin each kernel by itself.  Same conventions as the main header
 * (0 on success, ch_last_error(), device pointers, `stream` = hipStream_t as void*).
 */
#ifndef CONCEPTHASH_HIP_DEBUG_H
#define CONCEPTHASH_HIP_DEBUG_H

#include "concepthash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test / bench taps (not part of the product path): one fused-epilogue GEMM launch on caller buffers.  `variant` chooses the
 * kernel of that call alone (0 = the dispatcher's rule, 1 = 128x128 two-phase kernel, 2 = 256x256 ping-pong kernel, ...: the
 * table is ch_gemm_launch_variant in csrc/gemm_bf16.hip); no call changes what another call runs.
 * X [X_rows_alloc, K] bf16, W [N, K] bf16, bias [N] fp32; epi: 0 bias, 1 bias+quick_gelu, 2 bias+gelu,
 * 3 bias + (resid += v) + bf16 out, 4 resid += [addend bf16 [M,N]] + *scale_ptr * (acc + bias). */
int ch_debug_gemm(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias, int32_t M,
                  int32_t N, int32_t K, int32_t epi, void *out_bf16, int32_t ldo, float *resid, int32_t ldr,
                  const float *scale_ptr, const void *addend, void *stream);
/* The LayerNorm-fold epilogues: epi 6 = bias + row statistics of the bf16 output -> stats_out
 * [M, N/64, 2]; 7 = epi 4 + hb_out = bf16(resid) + its row statistics; 8/9/10 = y = rstd*(acc - mean*fold_c) + bias
 * [+ quick_gelu / gelu], mean/rstd from stats_in [M, K/64, 2] (partial sums of the rows of X) and ln_eps. */
int ch_debug_gemm_ln(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias, int32_t M,
                     int32_t N, int32_t K, int32_t epi, void *out_bf16, int32_t ldo, float *resid, int32_t ldr,
                     const float *scale_ptr, const void *addend, const float *stats_in, const float *fold_c, float ln_eps,
                     float *stats_out, void *hb_out, void *stream);
/* The training-step epilogues on caller buffers.  epi 11 / 12 = out_bf16 = s * bf16(acc + bias) * act'(aux) with act = quick_gelu
 * (11, s = 1) / exact GELU (12, s = *scale_ptr, or 1 when scale_ptr is null); aux [M, ldo] bf16 shares the layout of out_bf16 and must
 * not overlap it.  epi 13 / 14 = out_bf16 = the LayerNorm-folded linear of epi 8 and hb_out [M, ld_hb] = quick_gelu / GELU of the
 * rounded out_bf16.  variant: 0 = dispatcher, 1 = 128x128 two-phase, 2 / 4 = 256x256 ping-pong schedules, 7 = ring (which does not
 * carry these epilogues: an error). */
int ch_debug_gemm_train(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias, int32_t M, int32_t N,
                        int32_t K, int32_t epi, void *out_bf16, int32_t ldo, const void *aux, const float *scale_ptr,
                        const float *stats_in, const float *fold_c, float ln_eps, void *hb_out, int32_t ld_hb, void *stream);
/* One forward-epilogue launch (epi 0 .. 4, 6 .. 10 as in the two taps above) with every leading dimension and launch option explicit:
 * out_bf16 [M, ldo], resid [M, ldr], addend [M, ld_addend], hb_out [M, ld_hb]; nt_resid_opt / nt_out_opt: 0 = by tensor size, 1 = the
 * non-temporal instance, -1 = the default-policy instance; group_n_opt > 0: n-tiles per weight group; rev = 1: serpentine tile order;
 * splitk = 1 (variant 2 only): cut EVERY tile of the last partial round along K (the tap's own workspace).  variant: 0 = the dispatcher's
 * rule, 1 / 2 / 4 / 7 = that kernel reached THROUGH the dispatcher (its cache-policy choice, its checks and the non-temporal counters
 * apply); a kernel that does not take the shape or the epilogue is an error, never another kernel. */
int ch_debug_gemm_fwd(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, const float *bias, int32_t M, int32_t N,
                      int32_t K, int32_t epi, void *out_bf16, int32_t ldo, float *resid, int32_t ldr, const float *scale_ptr,
                      const void *addend, int32_t ld_addend, const float *stats_in, const float *fold_c, float ln_eps, float *stats_out,
                      void *hb_out, int32_t ld_hb, int32_t nt_resid_opt, int32_t nt_out_opt, int32_t group_n_opt, int32_t rev,
                      int32_t splitk, void *stream);
/* The patch-embedding epilogue (epi 5): row m = img * patches_per_img + patch of X W^T, plus pos[1 + patch] (pos [1 + patches_per_img, N]
 * fp32), goes to row img * tokens_per_img + 1 + patch of resid [*, ldr] fp32; every other row of resid is left alone. */
int ch_debug_gemm_patch(int32_t variant, const void *X, int64_t X_rows_alloc, const void *W, int32_t M, int32_t N, int32_t K, float *resid,
                        int32_t ldr, const float *pos, int32_t tokens_per_img, int32_t patches_per_img, void *stream);
/* 1 when the library was built with CH_BUILD_EXPERIMENTS=1: the non-dispatched experiment kernels (GEMM variants 3 / 5 / 6 of
 * the taps above, the fused adapter kernel behind CH_FUSED_ADAPTER=1 and ch_debug_adapter) exist; 0 in the product build, where
 * those taps return an error. */
int32_t ch_debug_experiments_built(void);
/* How many GEMMs the dispatcher has sent to the 128x128 (which = 0) / 256x256 ping-pong (which = 1) kernel since the
 * library was loaded, and how many launches ran the instance with the non-temporal fp32-residual read-modify-write (which = 2) /
 * the non-temporal bf16 output store (which = 3): lets a parity test prove which kernel produced the output it compared. */
int64_t ch_debug_gemm_dispatch_count(int32_t which);
/* Copy the first nbytes of one activation buffer of the model's workspace, as the last ch_encode / ch_encode_hidden call left
 * it, to `out` (device): which = 0 H fp32 [rows, D] | 1 Xn | 2 QKV [rows, 3D] | 3 AO | 4 A | 5 AD [rows, max(bpad, 128)] |
 * 6 F1 [rows, ffn] (1..6 bf16).  tools/stage_probe.py compares every stage of a layer with the rounding-emulating oracle. */
int ch_debug_copy_buffer(ch_model *m, int32_t which, void *out, int64_t nbytes, void *stream);
/* Let the debug GEMM taps use the split-K tail of the 256x256 kernel (off by default: a split tile sums its K slices in a
 * different order, so it is no longer bit-identical to the 128x128 kernel). */
void ch_debug_set_gemm_splitk(int32_t on);
/* One fused adapter call H += a + scale * (GELU(LN(a) Wd^T + bd) Wu^T + bu) on caller buffers (a [M,D] bf16, H [M,D] fp32,
 * Wd [b,D] fp32, Wu [D, roundup(b,128)] bf16 zero-padded); work_* are caller scratch for the LayerNorm-folded weights. */
int ch_debug_adapter(const void *A, float *H, int32_t M, int32_t D, int32_t b, const float *Wd, const float *bd,
                     const float *gamma, const float *beta, const void *Wu_bf16_padded, const float *bu, const float *scale,
                     void *work_wdf, float *work_c, float *work_d, int32_t dbg, void *stream);
/* qkv [B*ntok, 3*heads*64] bf16 (q | k | v) -> out [B*ntok, heads*64] bf16: softmax(q k^T / 8) v per (image, head). */
int ch_debug_attention(const void *qkv, int32_t B, int32_t ntok, int32_t heads, void *out, void *stream);
/* The same launch with every mode of the kernels (attention.hip, attention_stream.hip): cattn (optional) [B, heads, ncon, ntok - ncon - 1]
 * fp32 receives the softmax rows of the last `ncon` tokens over tokens 1 .. ntok - ncon - 1 (attn_cache[-1][:, :, -Q:, 1:-Q],
 * models/arch/coop.py:481-482); compact = 1: only token 0 and the last `ncon` tokens are queries, out is [B * (1 + ncon), heads*64];
 * kernel: 0 = by length (<= 288 tokens the LDS-resident kernel, longer the streaming one), 1 = resident, 2 = streaming. */
int ch_debug_attention_ex(const void *qkv, int32_t B, int32_t ntok, int32_t heads, void *out, float *cattn, int32_t ncon, int32_t compact,
                          int32_t kernel, void *stream);
/* The causal instance of the resident kernel (the text tower's): query q attends keys 0 .. q; 1 <= ntok <= 288. */
int ch_debug_attention_causal(const void *qkv, int32_t B, int32_t ntok, int32_t heads, void *out, void *stream);
/* Attention launches since the library was loaded: which = 0 forward resident, 1 forward streaming, 2 backward resident, 3 backward
 * streaming -- lets a test prove which kernel produced the output it compared. */
int64_t ch_debug_attention_dispatch_count(int32_t which);

/* 1 = the mAP scan passes read the gallery through scalar loads (the round-1 form) instead of 16-row VMEM blocks + DPP row broadcast:
 * same results bit for bit, kept as a cross-check of the row loops (tests/test_hamming_gpu.py).  Process-wide, tests only. */
void ch_debug_set_hamming_scalar_loads(int32_t on);

/* Kernel taps of the training step: see train_kernels.hip / attention_bwd.hip. */
int ch_debug_attention_bwd(const void *qkv, const void *dO, int32_t B, int32_t ntok, int32_t heads, void *dqkv, const float *dpext,
                           int32_t ncon, void *stream);
/* ... with the kernel chosen as in ch_debug_attention_ex. */
int ch_debug_attention_bwd_ex(const void *qkv, const void *dO, int32_t B, int32_t ntok, int32_t heads, void *dqkv, const float *dpext,
                              int32_t ncon, int32_t kernel, void *stream);
int ch_debug_wgrad(const void *A, int32_t lda, const void *Bm, int32_t ldb, int64_t rows, int64_t rows_alloc, int32_t N, int32_t K,
                   float *out, void *stream);
int ch_debug_ln_bwd(const void *dyg, const void *x, int64_t rows, int32_t D, float eps, const float *dres_in, float *dres_out,
                    void *out_b, void *xhat_out, void *stream);
int ch_debug_act(const void *g, const void *pre, int64_t n, int32_t act, const float *scale_ptr, int32_t backward, void *out,
                 void *stream);

/* The training step's row, reduction and gradient-assembly launchers of train_kernels.hip, one launch sequence each on caller buffers
 * (tests/test_train_rowkernels_gpu.py holds every one to an fp64 restatement, tests/train_kernels_ref.py).  bf16 buffers are void *.
 * hb_stats: hb = bf16(H), stats [rows, D/64, 2] = (sum, sum of squares) of the ROUNDED values per 64-column slice.
 * normalize_bf16: out = bf16((x - mean) * rstd) with (mean, rstd) from `stats`.  colsum: out[n] = sum_m A[m * lda + n].
 * reduce_partials_multi: host arrays of njobs (1..4) entries; out[j][i] = sum_c partial[j][c * 4 n4[j] + i].
 * transposes: dst[c * ld_dst + r] = bf16(src[r * ld_src + c] * (colscale ? colscale[c] : 1)).
 * adapter_refresh / adapter_grads: `nad` adapters `stride` floats apart in the arena ([ln_w D][ln_b D][down_w b*D][down_b b]
 * [up_w D*b][up_b D][scale 1]); the other arrays hold one slot per adapter.  fold_grads: W / dW / db are host arrays of nparts (1..3)
 * device pointers.  embed_bwd: X and dY are replaced in place.  The last five are the row moves and row sums of the concept tokens. */
int ch_debug_hb_stats(const float *H, int64_t rows, int32_t D, void *hb, float *stats, void *stream);
int ch_debug_normalize_bf16(const void *x, const float *stats, int64_t rows, int32_t D, float eps, void *out, void *stream);
int ch_debug_colsum(const void *A, int32_t is_f32, int32_t lda, int64_t rows, int32_t N, float *out, void *stream);
int ch_debug_reduce_partials_multi(int32_t njobs, const float *const *partial, float *const *out, const int32_t *nchunks, const int32_t *n4,
                                   void *stream);
int ch_debug_transpose_f32_to_bf16(const float *src, int32_t R, int32_t C, int32_t ld_src, const float *colscale, void *dst, int32_t ld_dst,
                                   void *stream);
int ch_debug_transpose_bf16(const void *src, int32_t R, int32_t C, int32_t ld_src, void *dst, int32_t ld_dst, void *stream);
int ch_debug_adapter_refresh(const float *params, int64_t stride, int32_t nad, int32_t D, int32_t b, int32_t bpad, void *down_wf, float *fold_c,
                             float *fold_d, void *up_w, void *up_wT, void *down_wgT, void *stream);
int ch_debug_adapter_grads(const float *G, const float *cu, const float *T, const float *cd, const float *params, int32_t D, int32_t b,
                           int32_t bpad, float *grads, int32_t nad, int64_t stride, void *stream);
int ch_debug_fold_grads(const float *T, const float *c, const float *gamma, const float *beta, int32_t D, int32_t nparts, int32_t rows_each,
                        const float *const *W, float *const *dW, float *const *db, float *dgamma, float *dbeta, void *stream);
int ch_debug_embed_bwd(float *X, float *dY, int32_t B, int32_t ntok, int32_t np, int32_t D, const float *cls_pos0, const float *ctx,
                       const float *gamma, float eps, void *dx_patch, void *stream);
int ch_debug_small_ln_bwd(const float *dy, const float *x, const float *gamma, int32_t rows, int32_t D, float eps, float *dx, void *stream);
int ch_debug_token_rows_sum(const float *dX, int32_t B, int32_t ntok, int32_t nrows, int32_t D, float *out, void *stream);
int ch_debug_concept_rows_sum(const float *dH, int32_t B, int32_t ntok, int32_t Q, int32_t D, float *out, void *stream);
int ch_debug_scatter_concept_rows(const float *dhf, int32_t B, int32_t ntok, int32_t Q, int32_t D, float *dH, void *dHb, void *stream);
int ch_debug_expand_head_rows(const void *src, int32_t is_f32, int32_t B, int32_t ntok, int32_t Q, int32_t D, void *dst, void *stream);
int ch_debug_gather_concept_rows(const float *H, int32_t B, int32_t ntok, int32_t Q, int32_t D, float *out, void *stream);

/* The forward row kernels (rowops.hip), the hashing head (head.hip) and the load-time folds (small_f32.hip), one launcher each on caller
 * buffers (tests/test_forward_kernels_gpu.py holds every one to an fp64 restatement, tests/forward_kernels_ref.py).
 * im2col: images [B, 3, image, image] fp32 (image_dtype 0) or bf16 (1) -> out [B * (image / patch)^2, Kp] bf16, column
 * c * patch^2 + ky * patch + kx, zeros from 3 * patch^2 up to Kp.  assemble_preln: H [B * ntok, D] is replaced in place (row 0 of an image
 * from cls_pos0, rows past np from ctx, pre-LayerNorm) and xn = bf16(LayerNorm(H)).  layernorm_bf16: kernel 0 = the launcher's rule
 * (up to 1024 features the 16-byte kernel, wider rows the generic one), 1 = 16-byte kernel, 2 = generic kernel.
 * gather_head_rows: out [B * (1 + ncon), D] = the CLS row and the last ncon rows of every image.
 * head: the arguments are the fields of HeadParams (csrc/kernels.h) in order; every output but out_codes may be null and is then not
 * computed; out_packed [B, ceil(nbit / 64)] uint64, out_logits_concept [Q, B, C]; the two workspaces are allocated by the tap.
 * small_*: y = act(x W^T + b) (act 1 = relu, b may be null); LayerNorm of fp32 rows; y = a + b; attention on packed qkv [T, 3P];
 * l2-normalised rows and (out_bin, optional) their signs / sqrt(cols).  convert_bf16: [rows, cols] -> [rows, cols_pad], zero padded.
 * bn_fold: scale = w / sqrt(var + eps), shift = b - mean * scale.  fold_ln: Wdf [bpad, D] = bf16(Wd * gamma), c = its row sums,
 * d = Wd beta + bd; rows b .. bpad - 1 are zero. */
int ch_debug_im2col(const void *images, int32_t image_dtype, int32_t B, int32_t image, int32_t patch, int32_t Kp, void *out, void *stream);
int ch_debug_assemble_preln(float *H, int32_t B, int32_t ntok, int32_t np, int32_t D, const float *cls_pos0, const float *ctx,
                            const float *pre_w, const float *pre_b, const float *ln_w, const float *ln_b, float eps, void *xn, void *stream);
int ch_debug_layernorm_f32(const float *x, int64_t rows, int32_t D, const float *w, const float *b, float eps, void *out, void *stream);
int ch_debug_layernorm_bf16(const void *x, int64_t rows, int32_t D, const float *w, const float *b, float eps, void *out, int32_t kernel,
                            void *stream);
int ch_debug_gather_head_rows(const float *H, int32_t B, int32_t ntok, int32_t ncon, int32_t D, float *out, void *stream);
int ch_debug_head(const float *H, int32_t B, int32_t ntok, int32_t D, int32_t Q, int32_t nbit, int32_t C, int32_t P, const float *hash_pe,
                  const float *hash_fc, const float *bn_scale, const float *bn_shift, const float *center_l2, const float *center_bin,
                  const float *concept_pe, const float *concept_cent_l2, const float *post_w, const float *post_b, const float *vis_proj,
                  float ln_eps, float *out_codes, void *out_packed, float *out_logits_cont, float *out_logits_bin, float *out_logits_concept,
                  float *out_hash_features, float *out_image_features, void *stream);
int ch_debug_small_linear(const float *x, int32_t rows, int32_t in_f, const float *W, const float *b, int32_t out_f, int32_t act, float *y,
                          void *stream);
int ch_debug_small_layernorm(const float *x, int32_t rows, int32_t D, const float *w, const float *b, float eps, float *y, void *stream);
int ch_debug_small_add(const float *a, const float *b, int64_t n, float *y, void *stream);
int ch_debug_small_mha(const float *qkv, int32_t T, int32_t P, int32_t heads, float *out, void *stream);
int ch_debug_small_l2norm(const float *x, int32_t rows, int32_t cols, float *out_l2, float *out_bin, void *stream);
int ch_debug_convert_bf16(const float *x, int64_t rows, int32_t cols, int32_t cols_pad, void *out, void *stream);
int ch_debug_bn_fold(const float *w, const float *b, const float *mean, const float *var, int32_t n, float eps, float *scale, float *shift,
                     void *stream);
int ch_debug_fold_ln(const float *Wd, const float *bd, const float *gamma, const float *beta, int32_t b, int32_t bpad, int32_t D, void *Wdf,
                     float *c, float *d, void *stream);

/* The two kernels that are the text tower's own (text_model.hip), through the launchers ch_text_encode's chain calls, on caller buffers
 * (tests/test_text_chain_gpu.py; references in tests/text_chain_ref.py).  D % 128 == 0, D <= 1280.  Device pointers only, and NO range
 * check of ids / eos (ch_text_encode checks its host arrays): every id must be a row of tok, every eos entry in [0, T).
 * text_embed: H[row] = tok[ids[row]] + pos[row % T] for row < rows (fp32, one addition).
 * text_pool: out[r] = LayerNorm(H[eos ? r * T + eos[r] : r]) for r < nrows, fp32 in and out (two-pass mean / variance). */
int ch_debug_text_embed(const int32_t *ids, int32_t rows, int32_t T, int32_t D, const float *tok, const float *pos, float *H, void *stream);
int ch_debug_text_pool(const float *H, const int32_t *eos, int32_t nrows, int32_t T, int32_t D, const float *w, const float *b, float eps,
                       float *out, void *stream);

/* Copy one of the centre arrays a model holds since ch_model_create to `out` (device): which = 0 `center` [C, center_dim] as ingested |
 * 1 center_l2 [C, nbit] (projected, l2-normalised) | 2 center_bin [C, nbit] (its signs / sqrt(nbit)).  tests/test_text_query_gpu.py
 * holds ch_model_project_text + the normalisation launch against 1 and 2, bit for bit. */
int ch_debug_model_centers(ch_model *m, int32_t which, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONCEPTHASH_HIP_DEBUG_H */
