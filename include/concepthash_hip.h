/*
 * concepthash_hip.h -- C-ABI of libconcepthash_hip.so (MI355X / gfx950).
 *
 * The reference (kamwoh/concepthash) is pure Python/PyTorch and exposes NO FFI/operator interface (SURVEY.md F1,
 * section 8b); its boundary is Python import paths.  This header is therefore the boundary *defined by this
 * project*: each entry point names the reference function(s) it replaces (paths relative to the reference root) and
 * is what a maintainer's ctypes stub binds.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; ch_last_error() gives the message (thread local);
 *     no C++ exception crosses the boundary.
 *   - all data pointers are DEVICE pointers owned by the caller unless a parameter says "host".
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work and never
 *     synchronise, allocate or free device memory (graph-capture safe) -- except ch_model_create/destroy.
 *   - integers are bit-exact by contract; floating point tolerances are stated in DESIGN.md / tests.
 *   - no hidden global state: the library reads NO environment variable; every tuning / test knob is state of one opaque handle
 *     (ch_model_set_option), the only process-wide switches are the test taps of concepthash_hip_debug.h.
 */
#ifndef CONCEPTHASH_HIP_H
#define CONCEPTHASH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): ch_encode / ch_train_forward take the layout of the concept-attention tap as an argument (ch_model_set_concept_attn_layers
 * is gone), ch_model_profile_end takes the capacity of the caller's arrays, ch_model_set_option / ch_model_get_option replace every
 * environment variable the library used to read.
 * 3 (late round 4): ch_image_desc gained `stride` and `flip` (56 bytes: the training transforms through ch_preprocess), ch_preprocess takes
 * `max_taps` (kernel selection); ch_tensor.data may be a device pointer; new entry points ch_jpeg_* (decode split), ch_io_file_sizes / ch_io_read_files (batch file reads). */
#define CH_ABI_VERSION 3

typedef struct ch_model ch_model; /* opaque: weights (bf16/fp32, device) + activation workspace */

typedef struct ch_model_config {
    int32_t image_size;  /* H == W of the input, e.g. 224 (pretrain resolution; no pos-embed interpolation) */
    int32_t patch;       /* 14 / 16 / 32 */
    int32_t dim;         /* D: ViT width (multiple of 64) */
    int32_t layers;      /* L */
    int32_t heads;       /* attention heads; dim / heads must be 64 */
    int32_t ffn;         /* MLP hidden width */
    int32_t adapter_dim; /* adapter bottleneck b (0 = no adapters) */
    int32_t ncontext;    /* Q: number of concept tokens */
    int32_t nbit;        /* total hash bits = Q * bits-per-concept */
    int32_t nclass;      /* C */
    int32_t proj_dim;    /* P: CLIP projection dim (concept-token generator width) */
    int32_t center_dim;  /* width of the `center` buffer (512 for CLIP text features) */
    int32_t upt_heads;   /* heads of the concept-token generator MHA (config upt_config.num_heads, 8) */
    int32_t act;         /* 0 = quick_gelu (OpenAI CLIP), 1 = exact gelu */
    int32_t max_batch;   /* largest B accepted by ch_encode (workspace is sized for it) */
    float ln_eps;        /* LayerNorm eps (1e-5) */
    float bn_eps;        /* BatchNorm1d eps (1e-5) */
} ch_model_config;

/* One named fp32 tensor, in host OR device memory (the library copies with hipMemcpyDefault: a model that already sits on the GPU
 * is ingested without a round trip through the host).  `name` is the reference state_dict key, e.g.
 * "backbone.vision_model.encoder.layers.0.self_attn.q_proj.weight", "hash_fc.weight", "hash_bn.running_var". */
typedef struct ch_tensor {
    const char *name;
    const float *data; /* host or device, fp32, contiguous, PyTorch layout */
    int64_t numel;
} ch_tensor;

int ch_abi_version(void);
const char *ch_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Encode
 * ------------------------------------------------------------------------------------------------------------- */

/* Replaces: model construction + BaseTrainer.load_model_state (trainers/base.py:195-197) + .to(device)
 * (trainers/base.py:57-71) for models.arch.coop.LGHWithFixedPrompt.  Copies/convert weights to the device (GEMM
 * operands -> bf16, everything else fp32), and folds the input-independent parts of the forward once, on the GPU:
 * forward_hash_query (models/arch/coop.py:413-427) -> concept tokens; get_center (coop.py:624-625) -> projected,
 * l2-normalised centres; BatchNorm1d eval (coop.py:559) -> per-bit affine.  Unknown/missing names are an error;
 * aliases (`adapter_params.*`, `trainable_params.*`) are ignored.  `text_projection.*` may be absent when `center` is already nbit wide
 * (LGHWithoutText.get_center: the centres as they are); ch_model_project_text then refuses the handle. */
int ch_model_create(const ch_model_config *cfg, const ch_tensor *tensors, int32_t ntensors, ch_model **out);
void ch_model_destroy(ch_model *m);
/* bytes of device memory held by the model (weights + workspace) */
size_t ch_model_device_bytes(const ch_model *m);

/* Tuning / test options of ONE model handle ("no hidden global state except an opaque handle").  Every call
 * made on the handle afterwards uses the new value; outputs are bit-identical for every setting except "ln_fold" (rounding points
 * move), "splitk" (summation order) and "attn_stream" (another kernel's rounding).  Unknown keys and out-of-range values are errors.
 *   "streams"       1..4   micro-batch launch chains of ch_encode on as many HIP streams (default 2; 1 = what a per-kernel profile wants)
 *   "ln_fold"       0/1    LayerNorm folded into the consumer GEMMs (default 1)
 *   "prune_last"    0/1    final layer past its attention on the rows the hashing head reads only (default 1)
 *   "pp_min_k"      >= 0   smallest K that goes to the 256x256 ping-pong GEMM (0 = dispatcher default: 512 and >= 128 tiles)
 *   "attn_stream"   0/1    1 = attention of <= 288 tokens also runs the streaming kernels, forward and backward (tests; default 0: up to 288
 *                          tokens per image the LDS-resident kernels, past them -- up to a 32 x 32 patch grid -- the streaming ones)
 *   "resid_nt"      -1/0/1 non-temporal read-modify-write of the fp32 residual: off / by tensor size (default) / on
 *   "nt_out"        -1/0/1 non-temporal stores of large bf16 GEMM outputs: off / by tensor size (default) / on
 *   "group_n"       >= 0   n-tiles per L2-resident weight group of the GEMM tile order (0 = host heuristic)
 *   "graph_max_batch" >= 0 ch_encode calls with B <= this value replay the launch chain as ONE captured hipGraph (images staged into a library
 *                          buffer, requested outputs copied out of staging buffers; first call per (B, dtype, output set) runs eagerly and
 *                          captures).  0 (default) = off: ch_encode then only enqueues kernels and is itself capturable by the caller.
 *                          Bit-identical outputs; measured NEUTRAL on MI355X (batch 8: 2.07 vs 2.09 ms -- small batches are bound by the
 *                          latency of one GEMM tile per launch on the GPU, not by host launch time), hence opt-in.
 *                          (read-only keys of ch_model_get_option: "graph_replays", "graph_captures", "last_chains")
 *   "splitk"        0/1    split-K tail of the 256x256 GEMM (default 0; allocates 64 MiB per chain on first use)
 *   "serpentine"    0/1    alternate the row direction of consecutive launches (default 0)
 *   "chain_auto"    0/1    with "streams" = 2: use ONE chain for batches of fewer than 5,600 token rows (batch <= 27 of ViT-B/16), where it
 *                          measures 2-5 % faster.  Default 1; 0 = always split.  Outputs are bit-identical.
 *   "small_kernel"  0..2   GEMMs of the 128x128 path: 0 = the four-stage ring kernel up to 8,192 rows (batch <= 40 of ViT-B/16: -7 % per
 *                          step at batch 8), the two-phase kernel above; 1 = two-phase always; 2 = ring always.  Outputs are bit-identical.
 *   "pp_sched", "fused_adapter", "gemm_rows", "wide_kernel"  experiment kernels: non-zero values need the experiments build
 *   "train_chains" 1..2, "train_chain_min_rows", "train_prune_last" 0/1, "train_batched_grads" 0/1   read by ch_trainer_create from the model it is created on */
int ch_model_set_option(ch_model *m, const char *key, int64_t value);
int ch_model_get_option(ch_model *m, const char *key, int64_t *value);

/* Replaces: LGHWithFixedPrompt.forward (models/arch/coop.py:524-598) as driven by
 * COOPTrainer.compute_features_one_batch (trainers/coop.py:59-71), eval mode.
 *   images        [B,3,H,W] NCHW, fp32 (image_dtype 0) or bf16 (image_dtype 1)
 *   out_codes     [B,nbit] fp32 pre-sign codes ("codes", coop.py:559)                      (required)
 *   out_packed    [B,W] uint64, W = ceil(nbit/64); bit i = codes[i] > 0 (little endian)   (optional, NULL)
 *   out_logits_cont / out_logits_bin [B,C] fp32 (coop.py:573-580)                          (optional)
 *   out_logits_concept [Q,B,C] fp32 (coop.py:269-276)                                      (optional)
 *   out_hash_features  [B,Q,D] fp32 raw last-layer concept-token states (coop.py:503-509) (optional)
 *   out_image_features [B,P] fp32 pooled CLS -> post-LN -> visual_projection (coop.py:498-501) (optional)
 *   out_concept_attn   [B,heads,Q,Np] fp32 last-layer attention of the Q concept tokens over the Np patch tokens
 *                      = attn_cache[-1][:, :, -Q:, 1:-Q] (coop.py:481-482; consumer models/loss/coop.py:164-176)  (optional)
 *   concept_attn_all_layers  layout of out_concept_attn, part of THIS call (no sticky state on the handle): 0 = the last layer only,
 *                      [B,heads,Q,Np]; 1 = EVERY layer, [L,B,heads,Q,Np], layer l = attn_cache[l][:, :, -Q:, 1:-Q] -- what the
 *                      `avg_attn` form of the attention-diversity loss averages (models/loss/coop.py:164-167,
 *                      `torch.stack(outputs['attn_cache']).mean(0)`) and the per-layer visualisations read
 *                      (models/arch/coop.py:481-482), without the (B, heads, N, N) maps ever being written.
 * B must be in [1, max_batch]. */
int ch_encode(ch_model *m, const void *images, int32_t image_dtype, int32_t B, float *out_codes,
              uint64_t *out_packed, float *out_logits_cont, float *out_logits_bin, float *out_logits_concept,
              float *out_hash_features, float *out_image_features, float *out_concept_attn, int32_t concept_attn_all_layers,
              void *stream);

/* Parity tap (tests only): run the encoder for `layer` layers (0 = embeddings + concept tokens + pre-LN) and copy the
 * fp32 residual stream [B*N, D], N = 1 + patches + Q, to out_hidden.  Mirrors `image_hidden_states[layer]`
 * (models/arch/coop.py:474-486). */
int ch_encode_hidden(ch_model *m, const void *images, int32_t image_dtype, int32_t B, int32_t layer,
                     float *out_hidden, void *stream);

/* Replaces: LGHWithFixedPrompt.get_center (models/arch/coop.py:624-625) on rows other than the model's own `center` buffer -- the
 * step from CLIP text features to the code space that a text query needs (the rows are
 * `sign(pooler_output)` of ch_text_encode, as trainers/orthohash.py:94-145 builds the centres).
 *   feats      [N, center_dim] fp32 device
 *   out_codes  [N, nbit] fp32 device: text_projection(feats), Linear or Sequential(Linear, ReLU, Linear) as the model was created
 * Runs the launches that folded the model's own centres at ch_model_create, so the model's `center` rows give bit for bit the
 * projected centres behind out_logits_cont / out_logits_bin.  Any N >= 1: the hidden rows of the two-layer form go through a buffer
 * of the handle in chunks, nothing is allocated per call (so one handle serves one stream at a time here, as it does in ch_encode).
 * A model created without text_projection is an error. */
int ch_model_project_text(ch_model *m, const float *feats, int64_t N, float *out_codes, void *stream);

/* ---- Training step of the adapters -----------------------------------------------------------
 * Replaces, for everything that touches the [B*N, *] activations: the forward and `loss.backward()` of
 * COOPTrainer.train_one_batch (trainers/coop.py:107-131) through CLIPEncoderLayerWithAdapter.forward
 * (models/layers/adapter.py:127-177) and Adapter.forward (:46-60), with the backbone frozen and the adapters trainable
 * (trainers/base.py:133-152, configs/model/concept_hash_final_v1_nosa_apt.yaml `backbone_lr_scale: 0`).  The concept-token
 * generator (4 tokens), the hashing head on [B,Q,D] and the loss stay with the caller's autograd, which passes
 * `concept_tokens` in, takes `hash_features` out, and exchanges their gradients.
 *
 * Adapter parameter arena (fp32, device, CALLER-owned; the optimizer updates it in place): adapters in (layer, adapter 1, adapter
 * 2) order, each  [adapter_layer_norm.weight D][.bias D][down_proj.weight b*D][down_proj.bias b][up_proj.weight D*b]
 * [up_proj.bias D][scale 1];  the gradient arena has the same layout and is OVERWRITTEN by ch_train_backward. */
typedef struct ch_trainer ch_trainer;
/* total floats of the adapter arena of this model (0 without adapters) */
int64_t ch_adapter_arena_numel(const ch_model *m);
/* Shares the frozen weights of `m` (which must outlive the trainer); allocates the per-layer saved activations for max_batch.
 * Reads the model's "train_*" options (ch_model_set_option) once, here. */
int ch_trainer_create(ch_model *m, int32_t max_batch, float *params, float *grads, ch_trainer **out);
void ch_trainer_destroy(ch_trainer *t);
int64_t ch_trainer_bytes(const ch_trainer *t);
/* Re-derive the bf16 / LayerNorm-folded / transposed working copies from the parameter arena(s): call after every optimizer step. */
int ch_trainer_refresh(ch_trainer *t, void *stream);
/* ---- Trainable backbone (`backbone_lr_scale != 0`, reference trainers/base.py:133-152: the whole vision_model in param group 0).
 * A second caller-owned fp32 device arena pair holds the backbone's master weights and receives their gradients.  Layout, per encoder
 * layer (state-dict names below `vision_model.encoder.layers.<l>.`):
 *   [layer_norm1.weight D][layer_norm1.bias D][self_attn.q_proj.weight D*D][.bias D][self_attn.k_proj.weight D*D][.bias D]
 *   [self_attn.v_proj.weight D*D][.bias D][self_attn.out_proj.weight D*D][.bias D][layer_norm2.weight D][layer_norm2.bias D]
 *   [mlp.fc1.weight ffn*D][.bias ffn][mlp.fc2.weight D*ffn][.bias D]
 * then the embedding side (names below `vision_model.`):
 *   [embeddings.class_embedding D][embeddings.patch_embedding.weight D*3*patch*patch]
 *   [embeddings.position_embedding.weight (Np+1)*D][pre_layrnorm.weight D][pre_layrnorm.bias D]
 * The position table is the one the forward ADDS, (image_size/patch)^2 + 1 rows: at a resolution other than the pretrain one the caller
 * stores the interpolated table there and applies the interpolation's adjoint to the gradient it gets back.  post_layernorm and
 * visual_projection are not part of the arena: no term of the training loss reads them (their gradient is None in the reference).
 * Both functions need only the configuration (no device): numel of the arena; offset (floats) and numel of one tensor, -1 = no such name. */
int64_t ch_backbone_arena_numel(const ch_model_config *cfg);
int64_t ch_backbone_arena_offset(const ch_model_config *cfg, const char *name, int64_t *numel);
/* ch_trainer_create with the backbone arena pair (both NULL = ch_trainer_create: frozen backbone, nothing more allocated or computed).
 * With them the forward reads working copies derived from `backbone_params` (ch_trainer_refresh; the model's own frozen weights are not
 * read), and ch_train_backward also OVERWRITES `backbone_grads` with the gradient of every tensor of the arena.  Needs dim, ffn and
 * the 64-padded 3*patch^2 to be multiples of 128. */
int ch_trainer_create_ex(ch_model *m, int32_t max_batch, float *params, float *grads, float *backbone_params, float *backbone_grads,
                         ch_trainer **out);
/* Forward in training mode (adapter dropout 0, as the reference configs have it).
 *   concept_tokens    [Q,D] fp32 device: forward_hash_query() output (models/arch/coop.py:413-427), before pre_layrnorm
 *   out_hash_features [B,Q,D] fp32: last-layer states of the concept tokens (coop.py:503-509)
 *   out_cls           [B,D] fp32 last-layer CLS states (optional, NULL)
 *   out_concept_attn  [B,heads,Q,Np] fp32 last-layer attention of the concept tokens over the patch tokens
 *                     = attn_cache[-1][:, :, -Q:, 1:-Q] (coop.py:481-482), what the attention-diversity term of the loss reads
 *                     (models/loss/coop.py:164-189)                                                    (optional, NULL)
 *   concept_attn_all_layers  as in ch_encode: 1 = out_concept_attn is [L,B,heads,Q,Np]; the trainer remembers the layout of its last
 *                     forward, and the matching ch_train_backward takes d_concept_attn in the same one */
int ch_train_forward(ch_trainer *t, const void *images, int32_t image_dtype, int32_t B, const float *concept_tokens,
                     float *out_hash_features, float *out_cls, float *out_concept_attn, int32_t concept_attn_all_layers, void *stream);
/* Backward of the last ch_train_forward: d_hash_features [B,Q,D] fp32 and (optional, NULL) d_concept_attn fp32 in the layout that
 * forward was called with ([B,heads,Q,Np] or [L,B,heads,Q,Np]; ignored when that forward had no out_concept_attn) in;
 * adapter gradients into the gradient arena, d_concept_tokens [Q,D] fp32 out. */
int ch_train_backward(ch_trainer *t, const float *d_hash_features, const float *d_concept_attn, float *d_concept_tokens, void *stream);
/* torch.optim.SGD.step (configs/optim/sgd.yaml; maximize False) over ONE flat fp32 array -- the adapter arena: d = g + weight_decay * p;
 * buf = d on the first step, else momentum * buf + (1 - dampening) * d; p -= lr * (nesterov ? d + momentum * buf : buf).
 * n must be a multiple of 4 (ch_adapter_arena_numel is padded by the caller if not). */
int ch_sgd_step(float *params, const float *grads, float *momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                float dampening, int32_t nesterov, int32_t first_step, void *stream);
/* torch.optim.Adam.step / AdamW.step (single-tensor form, amsgrad False, maximize False) over ONE flat fp32 array, `step` = 1 on the first
 * call: decoupled 0 (Adam): g += weight_decay * p;  decoupled 1 (AdamW): p *= 1 - lr * weight_decay;  then
 * exp_avg += (g - exp_avg) * (1 - beta1);  exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * g * g;
 * p -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps)      (eps outside the square root).
 * The scalar factors are formed in double, as torch's host code does.  n must be a multiple of 4. */
int ch_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, int32_t decoupled, int64_t step, void *stream);
/* Launch profiler for bench.py's roofline: between begin and end every kernel launch of ch_encode is bracketed by
 * HIP events on the caller's stream (capacity max_launches events; launches beyond it are not recorded).
 * ch_model_profile_end waits for the last recorded event and returns, per category, the summed launch durations
 * (ms), the number of launches and their algorithmic FLOPs; `ncat` is the capacity of the caller's three arrays and must be
 * >= CH_NCAT (a caller built against a header with fewer categories is refused instead of overrun). */
/* The *_PRUNED categories are the launches of the final layer behind its attention, which run on the B * (1 + Q) rows the hashing
 * head reads instead of all B * N token rows: kept apart so that every category is ONE problem shape. */
enum {
    CH_CAT_IM2COL = 0, CH_CAT_GEMM_PATCH, CH_CAT_ROWOPS, CH_CAT_GEMM_QKV, CH_CAT_ATTENTION, CH_CAT_GEMM_OUT,
    CH_CAT_GEMM_DOWN, CH_CAT_GEMM_UP, CH_CAT_GEMM_FC1, CH_CAT_GEMM_FC2, CH_CAT_HEAD, CH_CAT_ADAPTER,
    CH_CAT_ATTENTION_PRUNED, CH_CAT_GEMM_OUT_PRUNED, CH_CAT_GEMM_DOWN_PRUNED, CH_CAT_GEMM_UP_PRUNED, CH_CAT_GEMM_FC1_PRUNED,
    CH_CAT_GEMM_FC2_PRUNED, CH_CAT_END, CH_NCAT
};
int ch_model_profile_begin(ch_model *m, int32_t max_launches);
int ch_model_profile_end(ch_model *m, int32_t ncat, double *ms_per_cat, int64_t *launches_per_cat, double *flops_per_cat);

/* Algorithmic FLOPs of one image through ch_encode (SURVEY.md section 8d formula). */
double ch_model_flops_per_image(const ch_model *m);

/* ---------------------------------------------------------------------------------------------------------------
 * Pre-process  (replaces the CPU-worker transform chain of configs/dataset/cub200.yaml:31-47 -- torchvision
 * Resize(size, bicubic) -> CenterCrop(crop) -> ToTensor -> normalize -- as run by engine.dataloader, engine.py:41-54)
 * ------------------------------------------------------------------------------------------------------------- */

/* One decoded image inside the concatenated uint8 HWC (RGB, 3 bytes per pixel) buffer.  The derived integers follow
 * Python / torchvision rounding and are computed by the host (concepthash_amd/preprocess.py):
 *   nw, nh      size after Resize(size): shorter side = size, the other int(size * long / short);
 *   left, top   CenterCrop origin int(round((n - crop) / 2.0)) (round-half-even);
 *   row0, nrows source rows the vertical pass needs for the crop's rows; tmp_offset: byte offset of this image's
 *               [nrows, crop, 3] intermediate in the workspace.  nrows = 0: the kernels leave this image's output slot
 *               untouched (the host wrapper uses it for images whose down-scaling needs more than ch_preprocess_max_taps()
 *               filter taps and fills the slot itself).
 * The training transforms of the same configs (configs/dataset/cub200.yaml:13-23: RandomResizedCrop(crop, bicubic) ->
 * RandomHorizontalFlip -> ToTensor -> normalize) use the same kernels: (h, w) is then the SIZE OF THE BOX the host drew
 * (torchvision get_params; PIL crops the box, then resizes it as an image of its own), src_offset points at the box's first
 * pixel, stride = the full image's width, nh = nw = crop, top = left = 0, and flip mirrors the output columns
 * (PIL FLIP_LEFT_RIGHT after the resize). */
typedef struct ch_image_desc {
    int64_t src_offset; /* bytes from `pixels` to the first pixel that is read (the image's, or the crop box's) */
    int64_t tmp_offset;
    int32_t h, w, nh, nw, top, left, row0, nrows;
    int32_t stride;     /* pixels per source row; 0 = w */
    int32_t flip;       /* 1: output column x is written to crop - 1 - x */
} ch_image_desc;

/* pixels: device uint8; desc_device: device array of B descriptors; max_rows = max nrows over the batch;
 * max_taps: an upper bound of the horizontal pass's filter taps per output column over the batch's images with nrows > 0 --
 * Pillow's ksize = 2 * ceil(2 * max(w / nw, 1)) + 1 (w / nw in double precision) -- or 0 = not known.  It only selects kernels:
 * up to 16 taps (down-scaling up to 3.5x) with crop % 4 == 0, 4-byte-aligned `pixels` and workspace and a 16-byte-aligned `out`
 * run the dword forms of the two passes (3x faster on MI355X), anything else the byte forms; the results are the same bits;
 * mean3_host / std3_host: HOST float[3]; out: device NCHW [B,3,crop,crop], out_dtype 0 = fp32, 1 = bf16;
 * workspace: device bytes, >= sum of nrows * crop * 3.  Resampling is Pillow's two-pass 8-bit bicubic (22-bit fixed-point
 * coefficients, uint8 intermediate): the uint8 pixels are bit-equal to PIL's, the output to the CPU chain's. */
int ch_preprocess(const uint8_t *pixels, const ch_image_desc *desc_device, int32_t B, int32_t max_rows, int32_t max_taps,
                  int32_t crop, const float *mean3_host, const float *std3_host, void *out, int32_t out_dtype,
                  uint8_t *workspace, void *stream);
/* largest number of filter taps per output pixel the kernels hold (down-scaling factor up to ~15.5) */
int32_t ch_preprocess_max_taps(void);

/* TrivialAugmentWide training chain (reference configs/transforms/trivialaugment.yaml): Resize(resize, BILINEAR, shorter side) ->
 * RandomHorizontalFlip -> TrivialAugmentWide(bicubic, fill None) -> CenterCrop(crop) -> ToTensor -> normalize.  The random draws
 * (flip, op, signed magnitude) are made on the host by the loader; the host derives each image's op scalars as torchvision / Pillow
 * do (utils.transforms.ta_op_params).  One descriptor per image: */
typedef struct ch_augment_desc {
    int64_t src_offset; /* bytes from `pixels` to the image's first byte ([h, w, 3] uint8) */
    int64_t tmp_offset; /* bytes from the workspace to the horizontal pass's rows ([nrows, nw, 3]) */
    int64_t img_offset; /* bytes from the workspace to the resized, flipped image ([nh, nw, 3]) the op reads */
    int32_t h, w, nh, nw;
    int32_t top, left;  /* CenterCrop origin in the resized image */
    int32_t row0, nrows;/* source rows of the horizontal pass; nrows = 0: the kernels skip the image (the caller's host route) */
    int32_t flip;       /* 1: the resized image is mirrored (FLIP_LEFT_RIGHT) before the op */
    int32_t op;         /* TrivialAugmentWide op index: 0 Identity, 1 ShearX, 2 ShearY, 3 TranslateX, 4 TranslateY, 5 Rotate, 6 Brightness,
                           7 Color, 8 Contrast, 9 Sharpness, 10 Posterize, 11 Solarize, 12 AutoContrast, 13 Equalize */
    int32_t iparam;     /* Posterize: bits; Rotate: 0 = affine (m), 1 = copy, 2 = ROTATE_90, 3 = ROTATE_270, 4 = ROTATE_180 (Pillow's fast paths) */
    int32_t reserved;
    double fparam;      /* the enhancers' factor 1 + m; Solarize's threshold */
    double m[6];        /* the geometric ops: the inverse affine matrix Pillow's Image.transform receives */
} ch_augment_desc;

/* workspace bytes ch_preprocess_augment needs for B images whose descriptors ask for `image_bytes` = sum of (nrows + nh) * nw * 3
 * (the tmp / img offsets are the caller's, inside that range after the first ch_augment_workspace(B, 0) bytes) */
int64_t ch_augment_workspace(int32_t B, int64_t image_bytes);
/* desc_device: device array of B descriptors; max_rows = max nrows, max_nh = max nh, max_nw = max nw over the batch; out: NCHW
 * [B,3,crop,crop] fp32 (out_dtype 0) or bf16 (1), normalised as ch_preprocess does.  Resize is Pillow's two-pass 8-bit resampler with
 * the triangle (BILINEAR) filter; the ops restate Pillow's arithmetic (ImageEnhance's blend, ImageOps' tables, the bicubic affine
 * sampler, the 3x3 SMOOTH filter): the output equals the PIL chain's. */
int ch_preprocess_augment(const uint8_t *pixels, const ch_augment_desc *desc_device, int32_t B, int32_t max_rows, int32_t max_nh,
                          int32_t max_nw, int32_t crop, const float *mean3_host, const float *std3_host, void *out, int32_t out_dtype,
                          uint8_t *workspace, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * JPEG decode split  (replaces the decode half of the loader workers: `Image.open(path).convert("RGB")` in the dataset classes
 * that engine.dataloader drives, engine.py:41-54 -- PIL = libjpeg-turbo with its default settings: islow IDCT, fancy upsampling)
 *
 * Host threads do what is serial (marker parsing + Huffman entropy decode -> int16 coefficient blocks in pinned memory), the GPU does
 * what is data-parallel (dequantise + 8x8 inverse DCT + chroma upsampling + YCbCr -> RGB), writing decoded RGB bytes in the layout
 * ch_preprocess reads.  Integer arithmetic restated from libjpeg-turbo (jidctint.c, jdsample.c, jdcolor.c): the bytes are bit-equal
 * to Pillow's.  Files outside the supported subset get status != 0 and are decoded by the caller's host decoder (PIL, the
 * reference's own path); see csrc/jpeg_host.cpp for the subset (plain C++: the host half; csrc/jpeg.hip holds the kernels).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct ch_jpeg_desc {
    int64_t coef_offset;  /* int16 elements from the batch coefficient buffer to this image's first block */
    int64_t pix_offset;   /* bytes from `pixels` to this image's [height, width, 3] RGB output */
    int64_t plane_offset; /* bytes from the plane workspace to this image's component planes */
    int32_t width, height;
    int32_t ncomp;        /* 1 (grey, replicated to RGB as PIL's convert("RGB") does) or 3 (YCbCr) */
    int32_t hs, vs;       /* luma sampling factors: 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0); chroma is 1x1 */
    int32_t mcu_w, mcu_h; /* MCUs per row / column */
    int32_t status;       /* 0 = decoded by this path (baseline, extended-sequential and progressive Huffman files); 1 not a JPEG,
                             2 truncated (inside the headers, or -- set by ch_jpeg_entropy_decode -- inside the entropy-coded data), 3 lossless / arithmetic coding, or a progressive file whose scans leave DC or the first AC
                             coefficients above bit 0 (libjpeg smooths those; set by ch_jpeg_entropy_decode), 4 not 8 bit, 5 component
                             count, 6 sampling factors, 7 multi-scan sequential, 8 colour space, 9 tables, 10 smaller than 16x16,
                             11 corrupt entropy data, a data segment that ends before its last MCU included (set by ch_jpeg_entropy_decode),
                             12 more pixels than Pillow accepts (2 x MAX_IMAGE_PIXELS), 13 a block's coefficients outside the range
                             libjpeg's decoders agree on (csrc/jpeg_host.cpp: the domain; set by ch_jpeg_entropy_decode) */
    int32_t nblocks;      /* 8x8 blocks of all components = coefficient elements / 64 */
    int32_t reserved;
    uint16_t quant[3][64]; /* quantisation tables per component, natural (row-major) order */
} ch_jpeg_desc;

/* HOST: parse the headers of n files (files[i], lens[i]: host pointers / byte counts).  Fills desc[i] (sizes, sampling, tables,
 * status) and default back-to-back offsets; totals: int16 coefficient elements, output bytes, plane-workspace bytes.  The caller may
 * rewrite the three offsets (e.g. after sizing the slots of the files it decodes itself). */
int ch_jpeg_plan(const uint8_t *const *files, const int64_t *lens, int32_t n, ch_jpeg_desc *desc, int64_t *total_coef, int64_t *total_pix,
                 int64_t *total_plane);
/* HOST: Huffman-decode the entropy-coded segments of the files with status 0 on `nthreads` threads into coef_host (host memory,
 * ideally pinned; every block fully written, DC prediction undone, natural order; a progressive file's scans -- spectral selection and
 * successive approximation, ITU-T T.81 annex G -- are accumulated into the same blocks).  A corrupt stream sets that descriptor's status. */
int ch_jpeg_entropy_decode(const uint8_t *const *files, const int64_t *lens, int32_t n, ch_jpeg_desc *desc, int16_t *coef_host,
                           int32_t nthreads);
/* HOST: the same two calls for a batch whose files sit back to back in ONE buffer (what a `gpu_decode` loader worker hands over):
 * file i = data[offsets[i], offsets[i + 1]), offsets has n + 1 entries. */
int ch_jpeg_plan_packed(const uint8_t *data, const int64_t *offsets, int32_t n, ch_jpeg_desc *desc, int64_t *total_coef, int64_t *total_pix,
                        int64_t *total_plane);
int ch_jpeg_entropy_decode_packed(const uint8_t *data, const int64_t *offsets, int32_t n, ch_jpeg_desc *desc, int16_t *coef_host,
                                  int32_t nthreads);
/* HOST: the file reads of a batch, without Python in the loop and without worker processes (replaces what remains of the reference's
 * loader workers, engine.py:41-54, once decoding has left the CPU).  ch_io_file_sizes: stat every path; ch_io_read_files: file i ->
 * dst[offsets[i], offsets[i] + sizes[i]) on `nthreads` threads.  Status 3 + ch_last_error() names the file that failed. */
int ch_io_file_sizes(const char *const *paths, int32_t n, int64_t *sizes);
int ch_io_read_files(const char *const *paths, int32_t n, const int64_t *offsets, const int64_t *sizes, uint8_t *dst, int32_t nthreads);
/* GPU: coefficient blocks -> RGB bytes.  coef_dev: the coefficient buffer on the device; desc_dev / desc_host: the same n descriptors
 * on the device and on the host (the host copy sizes the launch); planes_ws: device workspace of total_plane bytes; pixels: device
 * output (total_pix bytes); images with status != 0 are skipped (their slots are the caller's to fill). */
int ch_jpeg_reconstruct(const int16_t *coef_dev, const ch_jpeg_desc *desc_dev, const ch_jpeg_desc *desc_host, int32_t n,
                        uint8_t *planes_ws, uint8_t *pixels, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Retrieve  (replaces the un-vendored utils.hashing.{calculate_mAP, calculate_pr_curve, get_hamm_dist}; call sites
 *            experiments/test_hashing.py:106-119,153-162, trainers/orthohash.py:362; definition: SURVEY.md 8c)
 * ------------------------------------------------------------------------------------------------------------- */

/* codes [rows,nbit] fp32 -> packed [rows,W] uint64; bit i = (codes[i] - threshold) > 0.  Replaces the sign() /
 * threshold step of calculate_mAP (ternary_threshold = 0 at every reference call site). */
int ch_pack_sign(const float *codes, int64_t rows, int32_t nbit, float threshold, uint64_t *out_packed, void *stream);

/* Full distance matrix (small problems / get_hamm_dist semantics, trainers/orthohash.py:362; in-repo twin
 * get_hd, trainers/orthohash.py:263-264): out[Qn,G] int32 = popcount(q xor g). */
int ch_hamming_dist(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t *out,
                    void *stream);

/* Top-k by ascending (distance, gallery index).  g_index_base is added to the local gallery row number (gallery
 * shards).  out_idx [Qn,k] int64 (global index, -1 when k > G), out_dist [Qn,k] int32 (-1 when k > G).
 * 1 <= k <= 128, 1 <= W <= 4.  workspace: ch_hamming_topk_workspace() bytes. */
size_t ch_hamming_topk_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k);
int ch_hamming_topk(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t k,
                    int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ch_hamming_topk with a bit mask: dist = popcount((q xor g) and mask), everything else -- ranking by ascending (distance, gallery
 * index), the -1 fill, g_index_base, 1 <= k <= 128, 1 <= W <= 4 and the workspace (ch_hamming_topk_workspace() bytes) -- as above.
 * mask_stride == W: q_mask is [Qn,W], one mask per query (e.g. the bits a query is confident of); mask_stride == 0: q_mask is [W],
 * shared by all queries (e.g. the sub-codes of chosen concepts).  Any other stride, or a NULL q_mask, is status 2.  Bits of the
 * last word past nbit must be zero in the codes or in the mask. */
int ch_hamming_topk_masked(const uint64_t *q, const uint64_t *q_mask, int32_t mask_stride, int64_t Qn, const uint64_t *g, int64_t G,
                           int32_t W, int32_t k, int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Weighted (asymmetric) Hamming ranking: the gallery stays binary, query i pays w_ij for a disagreement on bit j, w_ij being its own
 * |code| quantised to P = 4 or 8 bits (L = 2^P - 1):  a_ij = |codes[i,j]|, 0 where the value is not finite or bit j is cleared in the
 * mask; amax_i = max_j a_ij; w_ij = floor(a_ij L / amax_i + 0.5) evaluated in fp64 (all 0 when amax_i = 0; 0 for bits past nbit).
 * out_planes [Qn,P,W] uint64 (W = ceil(nbit / 64)): bit b of planes[i,p,w] = bit p of w_{i,64w+b}; out_wsum [Qn] int32 = sum_j w_ij,
 * the largest distance query i can reach (<= 256 * 255).  mask: NULL, [W] with mask_stride 0 or [Qn,W] with mask_stride W -- what
 * ch_hamming_topk_masked takes.  P outside {4, 8}, nbit outside [1, 256] or another stride: status 2. */
int ch_weight_planes(const float *codes, int64_t Qn, int32_t nbit, const uint64_t *mask, int32_t mask_stride, int32_t P,
                     uint64_t *out_planes, int32_t *out_wsum, void *stream);

/* Top-k by ascending (D, gallery index), D(i,g) = sum_p 2^p popcount((q_i xor g) and planes[i,p]) = sum_j w_ij [bit_j(q_i) != bit_j(g)]
 * with q = ch_pack_sign of the same codes and planes from ch_weight_planes.  out_dist is D; the -1 fill, g_index_base, 1 <= k <= 128
 * and 1 <= W <= 4 as in ch_hamming_topk; lists of several shards merge with ch_topk_merge (D < 2^16).  workspace:
 * ch_hamming_topk_weighted_workspace() bytes (it covers both P).  A gallery of more than 65,535 segments of 65,536 rows is status 2. */
size_t ch_hamming_topk_weighted_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k);
int ch_hamming_topk_weighted(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                             int32_t W, int32_t k, int64_t g_index_base, int64_t *out_idx, int32_t *out_dist,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Filtered search: the top-k among ADMITTED rows only.  Row r in [0, G) of THIS call's gallery is admitted for query i iff
 *     allow == NULL, or bit r & 63 of allow[r >> 6] is set: allow is uint64 [ceil(G / 64)], one bitmap for all queries, indexed by the
 *         row's position in this call's gallery (not by g_index_base + r); bits past G in its last word are ignored; and
 *     want == NULL, or want[i] < 0, or (grp(r) == want[i]) != exclude: want is int64 [Qn], grp(r) = group[r] where a plane group (int32
 *         [G], values >= 0) is given and g_index_base + r where group == NULL (a row is its own group: "not the query's own row"
 *         without storing anything); exclude is one flag per call, 0 = only that group, 1 = every group but it -- any other value is
 *         status 2.
 * The result is the unfiltered entry's restricted to admitted rows: the k smallest by ascending (distance, global index) with the
 * sibling's own distances, idx = dist = -1 behind them where fewer than k rows are admitted; with every row admitted it equals the
 * sibling's bit for bit, and lists of gallery shards (each with its own g_index_base, bitmap and slice of group) merge with
 * ch_topk_merge.  The filter is a predicate inside the scan: rows that are not admitted cost no list slot, nothing of size Qn x G is
 * written.  The filtered kernels hold a few more registers than their siblings and their segments follow their own figures, so each
 * entry has its own workspace function.
 * ch_hamming_topk_filtered adds the filter to ch_hamming_topk (q_mask == NULL; mask_stride is then ignored) and to
 * ch_hamming_topk_masked (q_mask and mask_stride as there). */
size_t ch_hamming_topk_filtered_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k);
int ch_hamming_topk_filtered(const uint64_t *q, const uint64_t *q_mask, int32_t mask_stride, int64_t Qn, const uint64_t *g, int64_t G,
                             int32_t W, int32_t k, int64_t g_index_base, const uint64_t *allow, const int32_t *group,
                             const int64_t *want, int32_t exclude, int64_t *out_idx, int32_t *out_dist, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ch_hamming_topk_weighted among admitted rows only: its arguments and distance D, plus the filter as described above.  The workspace
 * covers both P. */
size_t ch_hamming_topk_weighted_filtered_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k);
int ch_hamming_topk_weighted_filtered(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G,
                                      int32_t W, int32_t k, int64_t g_index_base, const uint64_t *allow, const int32_t *group,
                                      const int64_t *want, int32_t exclude, int64_t *out_idx, int32_t *out_dist, void *workspace,
                                      size_t workspace_bytes, void *stream);

/* Per-sub-code distances of retrieved hits: idx [Qn,k] int64 as written by ch_hamming_topk(_masked) / ch_topk_merge (global index =
 * gallery row + g_index_base, -1 = absent).  The code's first nbit bits are nsub equal sub-codes of nbit / nsub bits (sub-code c =
 * bits [c nbit/nsub, (c+1) nbit/nsub); it may straddle a 64-bit word); out [Qn,k,nsub] int32 = popcount of q xor g inside each, -1 in
 * all nsub slots of an absent hit.  nsub must divide nbit, nbit <= 64 W, 1 <= W <= 4.  The indices are checked on the host before
 * any row is read (one device-to-host copy of idx and a stream synchronisation): an index outside [g_index_base, g_index_base + G)
 * other than -1 is status 2 and nothing is launched. */
int ch_hamming_subcode_dist(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, const int64_t *idx, int32_t k,
                            int64_t g_index_base, int32_t nbit, int32_t nsub, int32_t *out, void *stream);

/* Merge nlists per-shard top-k lists ([nlists,Qn,k] each sorted ascending by (dist, idx); -1 entries = absent)
 * into the global top-k [Qn,k]. */
int ch_topk_merge(const int64_t *idx_lists, const int32_t *dist_lists, int32_t nlists, int64_t Qn, int32_t k,
                  int64_t *out_idx, int32_t *out_dist, void *stream);

/* Labels: single-label mode (LW == 0): int32 class id per row.  Multi-label mode (LW > 0): uint64[rows,LW] bitmasks;
 * relevant <=> masks intersect. */

/* mAP pass 1: per (gallery segment, query, distance bucket) counts.  The gallery is cut into nseg contiguous segments
 * of seg_rows rows (last one shorter); out_hist [nseg, Qn, nb, 2] uint32 with nb = 64*W+1, [..,0] = #rows at that
 * distance, [..,1] = #relevant rows.  seg_rows <= 65535. */
int ch_hamming_hist(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, const void *q_labels,
                    const void *g_labels, int32_t LW, int32_t seg_rows, uint32_t *out_hist, void *stream);

/* mAP pass 2: AP numerators in 2^-32 fixed point.  base [nseg,Qn,nb,2] uint32: for each (segment, query, bucket) the
 * number of rows / relevant rows ranked before the segment's first row of that bucket (global prefix over lower
 * buckets and over earlier segments -- and earlier gallery shards -- of the same bucket; built by
 * ch_hamming_hist_prefix or by the multi-GPU host code).  rank_limit = R (rows ranked after R do not count; <= 0: no
 * limit).  first_rel: NULL, or int32[Qn] = relevance (0/1) of each query's rank-1 row, which is then dropped before
 * ranking (remove_first_retrieved, experiments/test_hashing.py:105-112).  Accumulates (atomic add) into out_S[Qn]
 * uint64 and out_nrel[Qn] uint32 -- zero them first.  AP[q] = S[q] / (nrel[q] * 2^32). */
int ch_hamming_ap(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, const void *q_labels,
                  const void *g_labels, int32_t LW, int32_t seg_rows, const uint32_t *base, int64_t rank_limit,
                  const int32_t *first_rel, unsigned long long *out_S, uint32_t *out_nrel, void *stream);

/* The same pass for up to 16 rank limits at once (one gallery scan instead of one per limit): rank_limits[nlimits] is a
 * HOST array, ascending, entries <= 0 meaning "no limit" (they sort last); out_S [nlimits, Qn] uint64 and out_nrel
 * [nlimits, Qn] uint32 are accumulated row r under limit r.  With limits = the list R of calculate_mAP, the depths of
 * calculate_pr_curve (experiments/test_hashing.py:124-128,153-167) or the k of P@k / R@k -- out_nrel under limit k IS
 * the number of relevant rows in the top k -- every depth-dependent statistic of the evaluator comes out of one pass. */
int ch_hamming_ap_multi(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, const void *q_labels,
                        const void *g_labels, int32_t LW, int32_t seg_rows, const uint32_t *base,
                        const int64_t *rank_limits, int32_t nlimits, const int32_t *first_rel, unsigned long long *out_S,
                        uint32_t *out_nrel, void *stream);

/* Record form of the two passes: ONE distance scan.  ch_hamming_hist_rec is ch_hamming_hist that additionally leaves, for every
 * relevant (query, gallery row) pair, a record (distance, position inside its (segment, query, distance) bucket) in a per-lane list:
 * rec = uint2[ch_hamming_rec_workgroups() * rec_cap * ch_hamming_rec_block(W)], rec_cnt = uint32[nseg, Qn] (list lengths),
 * wg_flags = uint32[ch_hamming_rec_workgroups()], ZEROED by the caller, set to 1 for a (query tile, segment) workgroup in which
 * some list needed more than rec_cap entries.  ch_hamming_ap_rec then produces exactly what ch_hamming_ap_multi produces (same
 * arguments + the record buffers; out_S / out_nrel zeroed by the caller): it walks the lists -- G / C records per query instead of
 * G rows -- and redoes the flagged workgroups by the two-scan kernel, so the result does not depend on rec_cap.  Replaces the second
 * scan of calculate_mAP's ranking (experiments/test_hashing.py:114-119) where the label distribution lets the lists stay short. */
size_t ch_hamming_rec_workgroups(int64_t Qn, int64_t G, int32_t W, int32_t seg_rows);
int32_t ch_hamming_rec_block(int32_t W);
int ch_hamming_hist_rec(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, const void *q_labels,
                        const void *g_labels, int32_t LW, int32_t seg_rows, uint32_t *out_hist, void *rec, int32_t rec_cap,
                        uint32_t *rec_cnt, uint32_t *wg_flags, void *stream);
int ch_hamming_ap_rec(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, const void *q_labels,
                      const void *g_labels, int32_t LW, int32_t seg_rows, const uint32_t *base, const void *rec, int32_t rec_cap,
                      const uint32_t *rec_cnt, const uint32_t *wg_flags, const int64_t *rank_limits, int32_t nlimits,
                      const int32_t *first_rel, unsigned long long *out_S, uint32_t *out_nrel, void *stream);

/* Single-GPU helper: hist [nseg,Qn,nb,2] -> base (same shape) + totals[Qn,2] (rows, relevant rows overall). */
int ch_hamming_hist_prefix(const uint32_t *hist, int32_t nseg, int64_t Qn, int32_t nb, uint32_t *out_base,
                           uint32_t *out_totals, void *stream);

/* Ranked lists of any depth: writes the gallery rows out AT THEIR RANK.  Replaces what a caller of the un-vendored utils.hashing
 * takes from a full argsort of the distance matrix: the first K hits for any K (ch_hamming_topk stops at 128) and hash lookup, every
 * row within a Hamming radius.  base [nseg, Qn, nb, 2] as ch_hamming_hist_prefix builds it from ch_hamming_hist with the SAME seg_rows
 * (only [..,0], the row counts, is read; the histogram pass may run with labels of zeros).  Gallery row j of query i has the 0-based
 * rank of ascending (distance, gallery index); where rank < out_limit[i] the pass writes
 *     out_idx[out_start[i] + rank] = g_index_base + j,   out_dist[out_start[i] + rank] = popcount(q_i xor g_j).
 * out_start int64 [Qn], out_limit uint32 [Qn]: device arrays; the caller sizes out_idx / out_dist so that slots
 * out_start[i] .. out_start[i] + out_limit[i] - 1 exist, and pre-fills what it wants in the slots no row reaches (limit > G).
 * All integers: the result does not depend on seg_rows.  1 <= W <= 4, 1 <= seg_rows <= 65535, G < 2^32. */
int ch_hamming_rank_scatter(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t seg_rows,
                            const uint32_t *base, const int64_t *out_start, const uint32_t *out_limit, int64_t g_index_base,
                            int64_t *out_idx, int32_t *out_dist, void *stream);

/* Evaluation under the weighted distance (mAP@R, P@k, R@k of the ranking ch_hamming_topk_weighted serves), by rank counting.
 * For one query: key(g) = D(q, g) << 32 | global index of g (uint64, unique; ascending keys = ascending (D, gallery index)), D and
 * planes as in ch_hamming_topk_weighted, global index = g_index_base + gallery row, g_index_base >= 0 and g_index_base + G <= 2^32.
 * r_0 < r_1 < ... < r_{n-1}: the sorted keys of the query's relevant rows.  Every gallery row adds one to bins[pos], pos = #{j : r_j <
 * key(row)}; then rank(r_j) = sum_{b <= j} bins[b] (1-based) and its rank among the relevant rows is j + 1.  A row whose key exceeds
 * r_{n-1} would fall into bin n, which is never read and does not exist.  The lists of all queries share CSR buffers: offsets int64
 * [Qn + 1] (device), keys uint64 [total], bins uint32 [total], total = offsets[Qn].  Labels as for the mAP passes (LW == 0: int32 ids,
 * LW > 0: uint64 [rows, LW] bitmasks).  P in {4, 8}, 1 <= W <= 4, otherwise status 2.  Nothing of size Qn x G is written.
 *
 * ch_hamming_rank_collect, offsets == NULL: count[i] += the number of relevant rows of query i (count uint32 [Qn], zeroed by the caller;
 * q, planes and keys are not read).  With offsets (the exclusive prefix of those counts; count zeroed again): writes the keys of query
 * i's relevant rows into keys[offsets[i] .. offsets[i + 1]), in no particular order -- the caller sorts every slice ascending -- and
 * leaves the slice's fill in count[i]. */
int ch_hamming_rank_collect(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G, int32_t W,
                            const void *q_labels, const void *g_labels, int32_t LW, int64_t g_index_base, const int64_t *offsets,
                            uint32_t *count, uint64_t *keys, void *stream);

/* The Qn x G scan: bins[offsets[i] + pos] += 1 for every gallery row with key <= r_{n-1} (atomic adds: zero bins first; calls on
 * gallery segments or shards with their own g_index_base add into the same bins, in any order, with the same result).  keys: every
 * slice sorted ascending.  The gallery is cut into segments of seg_rows rows (at most 65,535 of them), one workgroup per (query,
 * segment); a query with an empty slice does no work.  A list of at most list_cap keys (1 <= list_cap <= 8192) is searched in LDS
 * (12 list_cap bytes per workgroup: pass the longest list, capped), a longer one in global memory -- the result does not depend on
 * list_cap or seg_rows. */
int ch_hamming_rank_count(const uint64_t *q, const uint64_t *planes, int32_t P, int64_t Qn, const uint64_t *g, int64_t G, int32_t W,
                          int64_t g_index_base, int32_t seg_rows, const int64_t *offsets, const uint64_t *keys, int32_t list_cap,
                          uint32_t *bins, void *stream);

/* AP from the bins: out_S [nlimits, Qn] uint64 and out_nrel [nlimits, Qn] uint32 as ch_hamming_ap_multi defines them (S = sum over the
 * relevant rows inside the limit of floor(relrank 2^32 / rank); rank_limits: host array, ascending, <= 0 = no limit, last, at most
 * 16), WRITTEN, not accumulated; out_total [Qn] int32 (may be NULL) = the query's relevant rows.  remove_first != 0: rank 1 is dropped
 * before ranking, as first_rel does for ch_hamming_ap: it is relevant iff rank(r_0) == 1 (frel); a relevant row at rank 1 is skipped,
 * every other row counts with rank - 1 and relrank - frel, and out_total loses frel.  A query with an empty slice gets zeros. */
int ch_hamming_rank_ap(int64_t Qn, const int64_t *offsets, const uint32_t *bins, const int64_t *rank_limits, int32_t nlimits,
                       int32_t remove_first, unsigned long long *out_S, uint32_t *out_nrel, int32_t *out_total, void *stream);

/* Ternary codes (the reference's `ternary_threshold`, configs/val.yaml): t_j = sign(x_j) where |x_j| > margin,
 * 0 otherwise (NaN gives 0), on BOTH sides.  Packed as two adjacent bit planes per row, [rows, 2, W] uint64, W = ceil(nbit / 64):
 * plane 0 (sign): bit j = t_j > 0; plane 1 (mask): bit j = t_j != 0; bits past nbit are zero in both.  The distance is
 *     K(q, g) = nbit - sum_j t_q,j t_g,j = nbit - popcount(mq & mg) + 2 popcount((sq ^ sg) & mq & mg),   an int32 in [0, 2 nbit]:
 * twice the matmul form 0.5 (nbit - q g^T) on ternary codes -- "half bits": a disagreement both sides are sure of costs
 * 2, a bit either side is unsure of 1, an agreement 0.  Every ranking below is ascending (K, gallery index); all integers, so no
 * result depends on how a gallery is segmented or sharded.  1 <= W <= 4 and 1 <= nbit <= 64 W everywhere, otherwise status 2.
 *
 * ch_pack_ternary: codes [rows,nbit] fp32 -> out_planes [rows,2,W], ONE launch for both planes.  nbit outside [1, 256], or a margin
 * that is negative or not finite: status 2. */
int ch_pack_ternary(const float *codes, int64_t rows, int32_t nbit, float margin, uint64_t *out_planes, void *stream);

/* Full matrix of K (small problems): q [Qn,2,W], g [G,2,W] -> out [Qn,G] int32. */
int ch_ternary_dist(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, int32_t *out, void *stream);

/* Top-k by ascending (K, gallery index) over a two-plane gallery; out_dist is K.  The -1 fill, g_index_base, 1 <= k <= 128 and
 * 1 <= W <= 4 as in ch_hamming_topk; lists of several shards merge with ch_topk_merge.  workspace: ch_ternary_topk_workspace() bytes.
 * Keys are K << 22 | row in segment (K takes 10 bits), so a segment holds at most 2^22 rows; a gallery of more than 65,535 segments
 * is status 2. */
size_t ch_ternary_topk_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k);
int ch_ternary_topk(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, int32_t k,
                    int64_t g_index_base, int64_t *out_idx, int32_t *out_dist, void *workspace, size_t workspace_bytes, void *stream);

/* ch_ternary_topk among admitted rows only: its arguments and distance K, plus the filter (allow, group, want, exclude) as described
 * at ch_hamming_topk_filtered; a row of the two-plane gallery is one row of the bitmap and of group. */
size_t ch_ternary_topk_filtered_workspace(int64_t Qn, int64_t G, int32_t W, int32_t k);
int ch_ternary_topk_filtered(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, int32_t k,
                             int64_t g_index_base, const uint64_t *allow, const int32_t *group, const int64_t *want, int32_t exclude,
                             int64_t *out_idx, int32_t *out_dist, void *workspace, size_t workspace_bytes, void *stream);

/* Evaluation under K by rank counting: ch_hamming_rank_collect and ch_hamming_rank_count with key(g) = K(q, g) << 32 | global index
 * of g over two-plane codes -- the same CSR buffers (offsets, count, keys, bins), the same offsets == NULL counting call, the same
 * list_cap and seg_rows guarantees, the same labels.  Their bins go to ch_hamming_rank_ap as they are. */
int ch_ternary_rank_collect(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, const void *q_labels,
                            const void *g_labels, int32_t LW, int64_t g_index_base, const int64_t *offsets, uint32_t *count,
                            uint64_t *keys, void *stream);
int ch_ternary_rank_count(const uint64_t *q, int64_t Qn, const uint64_t *g, int64_t G, int32_t W, int32_t nbit, int64_t g_index_base,
                          int32_t seg_rows, const int64_t *offsets, const uint64_t *keys, int32_t list_cap, uint32_t *bins,
                          void *stream);

/* Real-valued codes ("real-valued codes"): the rankings of the codes before sign().  Codes are fp32 [rows, n],
 * 1 <= n <= 256; metric: 0 = cosine, 1 = euclidean, 2 = dot; anything else, or n out of range, is status 2.  Ascending in
 *     dot:        D = -(q . g)
 *     euclidean:  D = sum_j (q_j - g_j)^2                    (squared, from the differences)
 *     cosine:     D = 1 - (q^ . g^),  x^ = x * (1 / sqrt(sum_j x_j^2)), sqrt and division correctly rounded; a zero row stays zero (D = 1)
 * each an fmaf chain over j = 0 .. n - 1 in this order from 0.0f, with the same bits in every entry below.  Every ranking is ascending
 * key = ord(D) << 32 | row index, ord(D) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), b = bits(D + 0.0f).  Inputs must be finite (the
 * Python wrapper refuses others; the kernels do not define them).
 *
 * ch_dense_prepare: codes [rows,n] -> the scan operand every other entry takes for q and g, ch_dense_prepared_bytes(rows, n) bytes:
 * rows in blocks of 64, dimension-major inside a block -- out[(r / 64) * n * 64 + j * 64 + r % 64] = x^_r,j (x for euclidean and dot);
 * the rows that fill the last block are zeros. */
size_t ch_dense_prepared_bytes(int64_t rows, int32_t n);
int ch_dense_prepare(const float *codes, int64_t rows, int32_t n, int32_t metric, float *out, void *stream);

/* Full matrix of D (small problems): prepared q (Qn rows), prepared g (G rows) -> out [Qn,G] fp32. */
int ch_dense_dist(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, float *out, void *stream);

/* Top-k by ascending (ord(D), row index) over a prepared gallery: out_idx [Qn,k] int64 = g_index_base + row, out_dist [Qn,k] fp32 = D;
 * slots past the end of the gallery hold -1 / +inf.  1 <= k <= 128; g_index_base + G <= 2^32.  seg_rows: gallery rows per segment of
 * the scan, 0 = ch_dense_topk_seg_rows(Qn, G) (no result depends on it); workspace: ch_dense_topk_workspace() bytes for the same
 * seg_rows.  Lists of gallery shards merge exactly by ascending (ord(D), index). */
int32_t ch_dense_topk_seg_rows(int64_t Qn, int64_t G);
size_t ch_dense_topk_workspace(int64_t Qn, int64_t G, int32_t k, int32_t seg_rows);
int ch_dense_topk(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, int32_t k, int64_t g_index_base,
                  int32_t seg_rows, int64_t *out_idx, float *out_dist, void *workspace, size_t workspace_bytes, void *stream);

/* Evaluation under D by rank counting: ch_hamming_rank_collect and ch_hamming_rank_count with key(g) = ord(D(q, g)) << 32 | global
 * index of g over prepared codes -- the same CSR buffers (offsets, count, keys, bins), the same offsets == NULL counting call, the
 * same list_cap and seg_rows guarantees, the same labels.  Keys use all 64 bits: sort them as UNSIGNED.  Their bins go to
 * ch_hamming_rank_ap as they are. */
int ch_dense_rank_collect(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, const void *q_labels,
                          const void *g_labels, int32_t LW, int64_t g_index_base, const int64_t *offsets, uint32_t *count, uint64_t *keys,
                          void *stream);
int ch_dense_rank_count(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, int64_t g_index_base,
                        int32_t seg_rows, const int64_t *offsets, const uint64_t *keys, int32_t list_cap, uint32_t *bins, void *stream);

/* Two-stage search ("two-stage"): order a shortlist of rows per query by D.  q [Qn,n] and g [G,n] are the RAW
 * row-major fp32 codes, NOT the prepared layout (a shortlisted row is one contiguous read); cosine normalises both sides on the fly
 * with the arithmetic of ch_dense_prepare, so D(q, g) has the bits ch_dense_dist gives for the pair under all three metrics.
 * cand [Qn,m] int64: global row ids, row = id - g_index_base; an id < 0 or a row outside [0, G) is an empty slot and is never
 * dereferenced (the -1 tails of ch_hamming_rank_scatter's lists are such slots).  out_idx / out_dist [Qn,k]: the k first of the m
 * candidates by ascending key = ord(D) << 32 | row, -1 / +inf past the filled slots; a row listed twice appears twice.
 * 1 <= k <= m <= 4096 (32 KB of keys in LDS per query); g_index_base + G <= 2^32. */
int ch_dense_rerank(const float *q, int64_t Qn, const float *g, int64_t G, int32_t n, int32_t metric, const int64_t *cand, int32_t m,
                    int32_t k, int64_t g_index_base, int64_t *out_idx, float *out_dist, void *stream);

/* Learned rotation ("learned rotation"): iterative quantisation of real-valued codes.  codes [rows,n] fp32
 * row-major, 1 <= n <= 256.  R is block-diagonal with blocks of `block` = s columns (s divides n) and is passed compact, [n,s] fp32
 * row-major: row b s + l holds R_b[l, :] (off-block entries do not exist).  The rotated entry of row i and output j of block b is the
 * chain acc = 0; for l = 0 .. s-1: acc = fmaf(codes[i, b s + l], R_b[l, j - b s], acc), in this order, in both entries: a row rotates
 * to the same bits alone or in a batch, in the step or in the rotate.  Sign: B = +1 where z > 0, else -1 (ch_pack_sign's rule).
 * ch_itq_step: ONE launch over the codes.  out_M [n,s] fp64, row j = sum_i B_ij codes[i, b s + .]; out_stats [2] fp64 =
 * {sum_ij |z_ij|, sum_i |z_i|_1 / (sqrt(n) |z_i|_2)} (a zero row adds 0 to the second).  Both WRITTEN.  Nothing of size rows x n is
 * written.  M is accumulated in fp32 inside a segment of seg_rows rows (1 .. 4096; 0: chosen here) in row order, the segments'
 * partials are added in fp64 in segment order; no atomics, so two calls on the same inputs give the same bits.  workspace:
 * ch_itq_step_workspace bytes, 8-byte aligned (as out_M and out_stats).  rows == 0: status 0, nothing launched, nothing written. */
size_t ch_itq_step_workspace(int64_t rows, int32_t n, int32_t block, int32_t seg_rows);
int ch_itq_step(const float *codes, int64_t rows, int32_t n, const float *R, int32_t block, int32_t seg_rows, double *out_M,
                double *out_stats, void *workspace, size_t workspace_bytes, void *stream);
/* out [rows,n] fp32 = the chain above. */
int ch_itq_rotate(const float *codes, int64_t rows, int32_t n, const float *R, int32_t block, float *out, void *stream);

/* Reduction ("reduction"): the moments a PCA of real-valued codes is fitted on, and the projection that applies
 * it.  codes [rows,n] fp32 row-major, 1 <= n <= 256; blocks of `block` = s columns (s divides n).  shift: fp32 [n] or NULL;
 * y = fl32(x - shift), one rounding (y = x under NULL).
 * ch_pca_moments: out_sum [n] fp64, sum[j] = sum_i y_ij; out_gram [n,s] fp64 or NULL (only the sums are wanted),
 * gram[b s + a, c] = sum_i y_{i, b s + a} y_{i, b s + c}.  Both WRITTEN.  Inside a segment of seg_rows rows (1 .. 4096; 0: chosen
 * here) every entry of gram is one fp32 chain in row order, acc = fmaf(y_a, y_c, acc), and a sum is a fixed tree of plain fp32 adds
 * (P = max(1, 256 / n) interleaved row-order chains, added in the order 0 .. P-1); the segments' partials are added in fp64 in segment
 * order.  No atomics: two calls on the same inputs give the same bits, and gram is exactly symmetric inside a block.  workspace:
 * ch_pca_moments_workspace bytes (with_gram: whether out_gram is given), 8-byte aligned (as out_sum and out_gram).  rows == 0:
 * status 0, nothing launched, nothing written. */
size_t ch_pca_moments_workspace(int64_t rows, int32_t n, int32_t block, int32_t seg_rows, int32_t with_gram);
int ch_pca_moments(const float *codes, int64_t rows, int32_t n, int32_t block, const float *shift, int32_t seg_rows, double *out_sum,
                   double *out_gram, void *workspace, size_t workspace_bytes, void *stream);
/* out [rows, blocks t] fp32, 1 <= t <= s.  A is block-structured and passed compact, [n,t] fp32 row-major: row b s + l holds A_b[l, :].
 * out[i, b t + j] is the chain acc = 0; for l = 0 .. s-1: acc = fmaf(fl32(codes[i, b s + l] - shift[b s + l]), A_b[l, j], acc), in
 * this order: a row projects to the same bits alone or in a batch, and with t == s and shift == NULL it is ch_itq_rotate's chain. */
int ch_pca_project(const float *codes, int64_t rows, int32_t n, int32_t block, const float *shift, const float *A, int32_t t, float *out,
                   void *stream);

/* Tie bracket: for every query and rank limit the smallest and the largest AP@R that ANY order of the rows sharing a Hamming distance
 * can give (the ranking of the passes above breaks such ties by gallery index; another implementation's sort need not).
 * bucket_counts [Qn, nb, 2] uint32, nb = 64 W + 1: rows / relevant rows of each query at each distance over the WHOLE gallery -- the
 * histogram of ch_hamming_hist / ch_hamming_hist_rec summed over its segments (and over gallery shards) by the caller; there is no
 * nseg argument.  rank_limits as for ch_hamming_ap_multi (host array, ascending, <= 0 = no limit, last, at most 16).  remove_first != 0:
 * rank 1 of the tie order is dropped first -- any row of the lowest non-empty bucket, relevant or not; the bracket covers both.
 * out_* [nlimits, Qn], WRITTEN (not accumulated): AP_low = S_low / (nrel_low * 2^32), AP_high likewise, in the fixed point of
 * ch_hamming_ap.  Inside the bucket a limit cuts every feasible number t of relevant rows inside the limit is a candidate (relevant
 * rows first is NOT always the maximum there, the denominator moves with t); candidates are compared as float64 AP, equal values
 * keep the smaller t, and an irrelevant dropped row is kept over a relevant one -- so the integers are deterministic.
 * bucket_counts (read as (rows, relevant) pairs), out_S_low and out_S_high must be 8-byte aligned (checked).
 * Cost: one fixed-point division per (query, relevant row, order), plus, for every limit that cuts a bucket holding both relevant and
 * irrelevant rows, about min(r, take)^2 / 2 more on the low side (r relevant rows in that bucket, take = rows of it inside the limit; every
 * candidate t is a sum of its own, run by ONE wave per query).  Measured up to r = 676 (0.9 ms for 16,384 queries x 1M rows).  A large
 * finite limit over few classes -- r and take in the tens of thousands -- is 1e7 .. 1e9 serial divisions per query and NOT measured:
 * split such a call, or ask for the unlimited bracket (<= 0: no bucket is cut, the cost is linear). */
int ch_hamming_tie_bracket(const uint32_t *bucket_counts, int64_t Qn, int32_t nb, const int64_t *rank_limits, int32_t nlimits,
                           int32_t remove_first, unsigned long long *out_S_low, uint32_t *out_nrel_low,
                           unsigned long long *out_S_high, uint32_t *out_nrel_high, void *stream);

/* Tie expectation: for every query the MEAN of AP@R, hits@k and R@k over every order of the rows sharing a Hamming distance, each
 * bucket independently and uniformly permuted -- the value that depends on no sort implementation; it lies inside
 * the bracket of ch_hamming_tie_bracket.  bucket_counts, rank_limits and remove_first as there (0 <= nlimits <= 16); ks: host array of
 * 0 <= nk <= 16 depths k >= 1, in any order.  remove_first != 0: the dropped rank-1 row is uniform among the rows of the lowest non-empty
 * bucket, and every output is the mixture of the two kinds of dropped row (the recall of a kind divides by the relevant rows it leaves).
 * out_ap [nlimits, Qn], out_hits [nk, Qn], out_recall [nk, Qn]: fp64, WRITTEN; a query without a gallery row, or without a relevant
 * one, gets zeros.  bucket_counts and the outputs must be 8-byte aligned (checked).
 * Arithmetic: fp64, one rounding per operation (no contraction); the hypergeometric weights of the bucket a limit cuts come from the
 * ratio recurrence outward from the mode, normalised by their sum, and a direction stops early only once the log-concave tail bound
 * w rho / (1 - rho) is under 2^-70.  |out - exact| is bounded per query by tests/tie_expected_ref.py `error_bound` (a few 1e-13 at a
 * few thousand rows per bucket).  Cost: one fp64 division per gallery row inside the largest limit plus, per limit that cuts a bucket,
 * one per row of that bucket inside the limit and a few per kept weight (about 20 standard deviations of the hypergeometric count):
 * linear, never take^2. */
int ch_hamming_tie_expected(const uint32_t *bucket_counts, int64_t Qn, int32_t nb, const int64_t *rank_limits, int32_t nlimits,
                            const int64_t *ks, int32_t nk, int32_t remove_first, double *out_ap, double *out_hits, double *out_recall,
                            void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * CLIP text tower (language-guided class centres)
 * ------------------------------------------------------------------------------------------------------------- */

/* Replaces: `CLIPModel.from_pretrained(model_id).text_model` as trainers/orthohash.py:94-145 (language_guided_codebook) runs it:
 * input_ids only (no attention mask: causality keeps the padding behind EOS away from it), `pooler_output` = the EOS token's row
 * after final_layer_norm, no text projection.  Forward only, once per training run. */
typedef struct ch_text ch_text; /* opaque: text-tower weights (bf16 GEMM operands, fp32 the rest) + activation workspace */

typedef struct ch_text_config {
    int32_t vocab;         /* rows of token_embedding */
    int32_t max_positions; /* rows of position_embedding (77); at most 288.  CLIP's 77 positions run the attention kernel's 96-key causal
                              instance (same occupancy as the image tower's); models with more than 128 positions are accepted but their
                              causal instances hold one wave per SIMD fewer (129-160) or spill as the plain 257-288 instance does */
    int32_t dim;           /* width (multiple of 128, at most 1280) */
    int32_t layers;
    int32_t heads;         /* dim / heads must be 64 */
    int32_t ffn;           /* MLP hidden width (multiple of 128) */
    int32_t act;           /* 0 = quick_gelu (OpenAI CLIP), 1 = exact gelu */
    int32_t max_batch;     /* largest B accepted by ch_text_encode (workspace is sized for max_batch * max_positions rows) */
    float ln_eps;          /* LayerNorm eps (1e-5) */
} ch_text_config;

/* Tensor names are the HF state_dict keys `text_model.embeddings.{token,position}_embedding.weight`,
 * `text_model.encoder.layers.N.{layer_norm1,layer_norm2,self_attn.{q,k,v,out}_proj,mlp.fc1,mlp.fc2}.{weight,bias}` and
 * `text_model.final_layer_norm.{weight,bias}` (`text_model.embeddings.position_ids`, an index buffer, is accepted and ignored).
 * Unknown or missing names are an error.  The config is validated before any device call. */
int ch_text_create(const ch_text_config *cfg, const ch_tensor *tensors, int32_t ntensors, ch_text **out);
void ch_text_destroy(ch_text *m);
size_t ch_text_device_bytes(const ch_text *m);
/* ids [B, T] and eos_pos [B] are HOST int32 arrays, validated here (0 <= id < vocab, 0 <= eos_pos < T, 1 <= B <= max_batch,
 * 1 <= T <= max_positions: a bad value is a status and a message, never an out-of-range read on the GPU) and copied to the device on
 * `stream` through a pinned buffer of the handle: the caller may free or reuse both arrays as soon as the call returns.  The staging
 * buffers and the activation workspace belong to the handle, so ONE handle must not be used from two streams (or threads) at the same
 * time; calls on one stream queue up as usual (a call waits on the host until the previous call's copy of its arrays has executed).  out_pooled [B, dim] fp32 (device) = final_layer_norm of row eos_pos[b] of prompt b; out_hidden (optional, device,
 * [B, T, dim] fp32) = final_layer_norm of every row (HF `last_hidden_state`). */
int ch_text_encode(ch_text *m, const int32_t *ids, const int32_t *eos_pos, int32_t B, int32_t T, float *out_pooled, float *out_hidden,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONCEPTHASH_HIP_H */
