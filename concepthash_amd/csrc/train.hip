// ch_trainer: the ConceptHash TRAINING step of the adapters -- forward with saved
// activations + backward through the frozen CLIP blocks, on the forward's GEMM / attention kernels plus train_kernels.hip
// and attention_bwd.hip.  Reference: trainers/coop.py:107-131 (train_one_batch: forward, criterion, loss.backward(),
// optimizer.step()), models/layers/adapter.py:46-60 (Adapter), :127-177 (CLIPEncoderLayerWithAdapter.forward),
// trainers/base.py:133-152 (what is trainable: the adapters + get_training_modules(); the backbone is frozen).
//
// Division of labour: this library owns everything that touches the [B*ntok, *] activations -- the 12
// encoder layers forward and backward, > 99.9 % of the step's FLOPs -- and the gradients of the 24 adapters.  The concept-token
// generator (4 tokens), the hashing head on [B, Q, D] and the loss are a few MFLOP; they stay on the host framework's autograd
// (concepthash_amd/training.py), which hands `concept_tokens` in and d(hash_features) back, and receives d(concept_tokens).
//
// Forward = the LN-fold layer of ch_encode -- ONE definition, ch_layer_forward in layer_forward.h, issued by both -- with every
// layer's operands kept in buffers of its own: bf16(H) + row statistics (the LayerNorm inputs), qkv, attention output, a / m
// (sub-block outputs) + statistics, adapter pre-activations and activations, fc1 pre-activation.  Pre-activations are saved
// instead of activations: handing the layer a pre-activation buffer selects the epilogue that writes the pre-activation AND its
// activation; backward multiplies by the activation's derivative in the dgrad GEMM's epilogue (EPI_BIAS_DACT_*).  Layer 0's
// LayerNorm input comes from ch_hb_stats (ch_encode's layer 0 reads rows already normalised instead).
// Backward per layer, dH = gradient of the residual stream (fp32, bf16 copy dHb as the GEMM operand):
//   adapter:  G = dHb^T g, cu = colsum(dH)                                [weight-gradient products, up]
//             dpre = s (dHb W_up) o gelu'(pre)                            [dgrad GEMM + act_bwd]
//             d(branch input) = dH + LN_bwd(dpre (W_dn o gamma))          [dgrad GEMM with gamma folded into W^T + ln_bwd, which
//                                                                          also emits x_hat of the adapter input as bf16]
//             T = dpre^T x_hat, cd = colsum(dpre)                         [weight-gradient products, down]
//   MLP:      dF = (dM W_fc2) o act'(pre), dh = dF (W_fc1 o gamma2), dH += LN_bwd(dh)
//   attn:     dctx = dA W_o, dqkv = attention_bwd(qkv, dctx), dh = dqkv (W_qkv o gamma1), dH += LN_bwd(dh)
// Parameter arena (fp32, caller-owned, device): adapters in (layer, adapter) order, each
//   [ln_w D][ln_b D][down_w b*D][down_b b][up_w D*b][up_b D][scale 1];  the gradient arena has the same layout.
#include <algorithm>
#include <string>
#include <vector>

#include "layer_forward.h"
#include "model_internal.h"

namespace {
struct AdWork {
    bf16_t *down_wf = nullptr, *up_w = nullptr, *up_wT = nullptr, *down_wgT = nullptr;
    float *fold_c = nullptr, *fold_d = nullptr;
};
struct LayerT {
    bf16_t *qkv_wgT = nullptr, *out_wT = nullptr, *fc1_wgT = nullptr, *fc2_wT = nullptr;
};
// trainable backbone: the forward's working copies of one layer, derived from the fp32 arena by ch_trainer_refresh (biases and
// LayerNorm vectors are read from the arena itself)
struct BbWork {
    bf16_t *qkv_wf = nullptr, *out_w = nullptr, *fc1_wf = nullptr, *fc2_w = nullptr;
    float *qkv_c = nullptr, *qkv_d = nullptr, *fc1_c = nullptr, *fc1_d = nullptr;
};
// one layer's tensors inside the backbone arena (parameters or gradients): the layout written in include/concepthash_hip.h
struct BbPtr {
    float *ln1_w, *ln1_b, *qkv_w[3], *qkv_b[3], *out_w, *out_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};
struct BbEmb {
    float *cls, *patch_w, *pos, *pre_w, *pre_b;
};
struct Saved {
    bf16_t *Xn1, *QKV, *AO, *A, *P1, *G1, *Xn2, *F1pre, *A2, *P2, *G2;
    float *st1, *stA, *st2, *stA2;
};
}  // namespace

constexpr int TR_CHAINS = 2;

struct ch_trainer {
    ch_model *m = nullptr;
    int max_batch = 0, B = 0;
    // Two micro-batch chains on two streams (as ch_encode does), model option "train_chains" (default 2): chain 1 owns
    // its own row region of every activation buffer (so that padding rows never alias the other chain's data), its own weight-gradient
    // scratch and its own gradient arena; the two arenas are added once at the end (the assembly is linear in the weight-gradient
    // products).  A trainer created with two chains decides per step: two when one chain's N = D GEMMs would need more than one round
    // of tiles (or by "train_chain_min_rows"), else one -- the rule and its measurements are at ch_train_forward.
    int nchains = 1, nc = 1, Bc[TR_CHAINS] = {0, 0};
    int64_t chain_min_rows = 12000;
    int64_t row_off[TR_CHAINS] = {0, 0}, prow_off[TR_CHAINS] = {0, 0}, region_rows[TR_CHAINS] = {0, 0}, region_prows[TR_CHAINS] = {0, 0};
    ChDeviceOwner own;   // every device block, the aux stream and the fork / join events (ch_trainer_bytes = own.bytes())
    ChForkJoin fj;
    float *params = nullptr, *grads = nullptr, *grads1 = nullptr;
    int64_t ad_numel = 0;
    std::vector<AdWork> ad;     // [L * 2]
    std::vector<LayerT> lt;     // [L]
    std::vector<Saved> sv;      // [L]
    float *H = nullptr, *dH = nullptr, *ctx = nullptr;
    // final-layer row pruning (as ch_encode): past the last attention only CLS + the Q concept tokens of
    // every image are carried, forward and backward -- the loss reads nothing else, so every other row's gradient is zero there
    bool prune_last = true;
    int64_t hc_rows = 0;
    float *Hc = nullptr, *dHc = nullptr;
    bf16_t *dHcb = nullptr;
    bf16_t *dHb = nullptr, *dMb = nullptr, *tD = nullptr, *tD2 = nullptr, *tB = nullptr, *tM = nullptr, *tQKV = nullptr, *F1act = nullptr,
           *PATCH = nullptr, *XnDummy = nullptr;
    float *stDummy = nullptr;
    float *ws_wgrad[TR_CHAINS] = {}, *ws_colsum[TR_CHAINS] = {}, *G[TR_CHAINS] = {}, *T[TR_CHAINS] = {}, *cu[TR_CHAINS] = {},
          *cd[TR_CHAINS] = {}, *dctx_sum[TR_CHAINS] = {};
    // batched gradient assembly (model option "train_batched_grads"): the four chunk-slab sets of an adapter live side by side and are
    // reduced by ONE launch into that adapter's slot of Gs / Ts / cus / cds; the gradients of all 2 L adapters are assembled by one
    // launch pair at the end of the backward chain
    bool batched_grads = true;
    float *ws_wgradT[TR_CHAINS] = {}, *ws_colsumD[TR_CHAINS] = {}, *Gs[TR_CHAINS] = {}, *Ts[TR_CHAINS] = {}, *cus[TR_CHAINS] = {},
          *cds[TR_CHAINS] = {}, *ws_ag[TR_CHAINS] = {};
    // ---- trainable backbone (ch_trainer_create_ex with a second arena pair; everything below is unused, and nothing of it allocated,
    // for a trainer created by ch_trainer_create).  The forward reads `lw` / `patch_w` / `pos` / ...: the model's frozen weights, or --
    // trainable -- the working copies in `bw` and the arena's own biases and LayerNorm vectors.
    bool bb = false;
    float *bparams = nullptr, *bgrads = nullptr, *bgrads1 = nullptr;
    int64_t bb_numel = 0, bb_layer_numel = 0;
    std::vector<LayerW> lw;     // [L]
    std::vector<BbWork> bw;     // [L]
    const bf16_t *patch_w = nullptr;
    const float *pos = nullptr, *cls_pos0 = nullptr, *pre_w = nullptr, *pre_b = nullptr;
    bf16_t *bb_patch_w = nullptr;
    float *bb_cls_pos0 = nullptr;
    float *ws_bb[TR_CHAINS] = {}, *ws_bbcol[TR_CHAINS] = {}, *Tbb[TR_CHAINS] = {}, *cbb[TR_CHAINS] = {};
    bool forward_done = false;
    bool attn_all_layers = false;   // layout of the concept-attention tap, latched by ch_train_forward for the matching ch_train_backward
};

namespace {

void *talloc(ch_trainer *t, size_t bytes, bool &ok) {
    if (!ok) return nullptr;   // after a failure nothing more is allocated; the first error string stands
    void *p = t->own.alloc(bytes, true);
    if (!p) ok = false;
    return p;
}

int64_t adapter_numel(const ch_model_config &c) {
    const int64_t D = c.dim, b = c.adapter_dim;
    return 2 * D + b * D + b + D * b + D + 1;
}

// backbone arena layout (include/concepthash_hip.h): per layer
//   [ln1.w D][ln1.b D][q.w D*D][q.b D][k.w D*D][k.b D][v.w D*D][v.b D][out.w D*D][out.b D][ln2.w D][ln2.b D][fc1.w M*D][fc1.b M][fc2.w D*M][fc2.b D]
// then [class_embedding D][patch_embedding.weight D*3*p*p][position_embedding.weight (np+1)*D][pre_layrnorm.weight D][.bias D]
int64_t bb_layer_numel(const ch_model_config &c) {
    const int64_t D = c.dim, M = c.ffn;
    return 4 * D * D + 2 * D * M + 9 * D + M;
}
int64_t bb_emb_numel(const ch_model_config &c) {
    const int64_t D = c.dim, g = c.image_size / c.patch;
    return D + D * 3 * c.patch * c.patch + (g * g + 1) * D + 2 * D;
}
BbPtr bb_ptrs(float *base, const ch_model_config &c) {
    const int64_t D = c.dim, M = c.ffn;
    BbPtr p;
    float *q = base;
    auto take = [&](int64_t n) { float *r = q; q += n; return r; };
    p.ln1_w = take(D); p.ln1_b = take(D);
    for (int j = 0; j < 3; ++j) { p.qkv_w[j] = take(D * D); p.qkv_b[j] = take(D); }
    p.out_w = take(D * D); p.out_b = take(D);
    p.ln2_w = take(D); p.ln2_b = take(D);
    p.fc1_w = take(M * D); p.fc1_b = take(M);
    p.fc2_w = take(D * M); p.fc2_b = take(D);
    return p;
}
BbEmb bb_emb_ptrs(float *arena, const ch_model_config &c) {
    const int64_t D = c.dim, g = c.image_size / c.patch;
    BbEmb e;
    e.cls = arena + bb_layer_numel(c) * c.layers;
    e.patch_w = e.cls + D;
    e.pos = e.patch_w + D * 3 * c.patch * c.patch;
    e.pre_w = e.pos + (g * g + 1) * D;
    e.pre_b = e.pre_w + D;
    return e;
}

struct AdPtr {
    float *ln_w, *ln_b, *down_w, *down_b, *up_w, *up_b, *scale;
};
AdPtr ad_ptrs(float *base, const ch_model_config &c) {
    const int64_t D = c.dim, b = c.adapter_dim;
    AdPtr p;
    p.ln_w = base;
    p.ln_b = p.ln_w + D;
    p.down_w = p.ln_b + D;
    p.down_b = p.down_w + b * D;
    p.up_w = p.down_b + b;
    p.up_b = p.up_w + D * b;
    p.scale = p.up_b + D;
    return p;
}

// a ChGemmCall (layer_forward.h) as GemmParams, with the per-model options the training step honours
int gemm(ch_trainer *t, int chain, int rows, const ChGemmCall &g, hipStream_t s, int64_t x_rows_alloc = 0) {
    const int D = t->m->cfg.dim;
    GemmParams p{};
    p.X = g.X; p.W = g.W; p.M = rows; p.N = g.N; p.K = g.K; p.X_rows_alloc = x_rows_alloc ? x_rows_alloc : t->region_rows[chain];
    p.bias = g.bias; p.out_bf16 = g.out; p.ldo = g.ldo; p.resid = g.resid; p.ldr = D; p.scale_ptr = g.scale; p.addend = g.addend;
    p.ld_addend = D; p.stats_in = g.stats_in; p.fold_c = g.fold_c; p.ln_eps = g.eps; p.stats_out = g.stats_out; p.hb_out = g.hb_out;
    p.ld_hb = g.ld_hb ? g.ld_hb : D; p.aux = g.aux; p.pp_min_k = t->m->pp_min_k;
    p.nt_resid_opt = t->m->resid_nt; p.nt_out_opt = t->m->nt_out; p.group_n_opt = t->m->group_n; p.wide_opt = t->m->wide_kernel;
    return ch_gemm_bf16(p, g.epi, s);
}

// the row region of chain `ch`: every activation buffer is addressed through these
struct Rows {
    int64_t r0;
    int D, M, bpad;
    template <typename T>
    T *d(T *p) const { return p + r0 * D; }
    template <typename T>
    T *d3(T *p) const { return p + r0 * 3 * D; }
    template <typename T>
    T *m(T *p) const { return p + r0 * M; }
    template <typename T>
    T *b(T *p) const { return p + r0 * bpad; }
    float *st(float *p) const { return p + r0 * (D / 64) * 2; }
};

// the training step's launcher of one chain's forward layers (layer_forward.h)
struct TrainLaunch {
    ch_trainer *t;
    int ch, B;
    hipStream_t s;
    int gemm(int rows, const ChGemmCall &g) { return ::gemm(t, ch, rows, g, s); }
    int attention(const bf16_t *qkv, bf16_t *out, float *cattn, bool compact) {
        const ch_model *m = t->m;
        return ch_attention(qkv, B, m->ntok, m->cfg.heads, out, s, cattn, m->cfg.ncontext, compact, false, m->attn_stream ? 2 : 0);
    }
    int gather_head_rows(const float *H, float *Hc) { return ch_gather_head_rows(H, B, t->m->ntok, t->m->cfg.ncontext, t->m->cfg.dim, Hc, s); }
};

int forward_chain(ch_trainer *t, int ch, const void *images_all, int image_dtype, int img0, int B, float *out_hf_all, float *out_cls_all,
                  float *out_cattn_all, hipStream_t s) {
    ch_model *m = t->m;
    const ch_model_config &c = m->cfg;
    const int D = c.dim, M = c.ffn, ntok = m->ntok, np = m->np, bpad = m->bpad, Q = c.ncontext, L = c.layers;
    const int rows = B * ntok;
    const Rows R{t->row_off[ch], D, M, bpad};
    float *H = R.d(t->H);   // the residual stream; re-pointed at the compact copy past the last layer's attention
    bf16_t *PATCH = t->PATCH + t->prow_off[ch] * m->Kp;
    const size_t img_elems = (size_t)3 * c.image_size * c.image_size;
    const void *images = (const char *)images_all + (size_t)img0 * img_elems * (image_dtype == 0 ? 4 : 2);
    // ---- embeddings (models/arch/coop.py:452-472): im2col + patch GEMM, CLS / position / concept tokens, pre-LN
    if (int e = ch_im2col(images, image_dtype, B, c.image_size, c.patch, m->Kp, PATCH, s)) return e;
    {
        GemmParams p{};
        p.X = PATCH; p.W = t->patch_w; p.M = B * np; p.N = D; p.K = m->Kp; p.X_rows_alloc = t->region_prows[ch];
        p.resid = H; p.ldr = D; p.pos = t->pos; p.tokens_per_img = ntok; p.patches_per_img = np; p.pp_min_k = m->pp_min_k;
        if (int e = ch_gemm_bf16(p, EPI_PATCH, s)) return e;
    }
    const LayerW &w0 = t->lw[0];
    if (int e = ch_assemble_preln(H, B, ntok, np, D, t->cls_pos0, t->ctx, t->pre_w, t->pre_b, w0.ln1_w, w0.ln1_b, c.ln_eps,
                                  R.d(t->XnDummy), s))
        return e;
    if (int e = ch_hb_stats(H, rows, D, R.d(t->sv[0].Xn1), R.st(t->sv[0].st1), s)) return e;
    const int nq = 1 + Q;
    float *Hc = t->Hc + (size_t)ch * t->hc_rows * D;
    TrainLaunch run{t, ch, B, s};
    ChChain st{B, ntok, Q, D, M, bpad, c.adapter_dim, c.act, c.ln_eps, rows, H};
    for (int l = 0; l < L; ++l) {
        const Saved &v = t->sv[l];
        const bool last = l == L - 1;
        // every operand is kept per layer for backward, pre-activations included; only fc1's activation is scratch, and the bf16(H)
        // that nothing follows goes to the dummies
        ChLayerBufs b{};
        b.Xn1 = R.d(v.Xn1); b.st1 = R.st(v.st1); b.qkv_folded = true;
        b.QKV = R.d3(v.QKV); b.AO = R.d(v.AO); b.A = R.d(v.A); b.stA = R.st(v.stA); b.A2 = R.d(v.A2); b.stA2 = R.st(v.stA2);
        b.AD[0] = R.b(v.G1); b.ADpre[0] = R.b(v.P1); b.AD[1] = R.b(v.G2); b.ADpre[1] = R.b(v.P2);
        b.Xn2 = R.d(v.Xn2); b.st2 = R.st(v.st2); b.F1 = R.m(t->F1act); b.F1pre = R.m(v.F1pre);
        b.Xn_next = R.d(last ? t->XnDummy : t->sv[l + 1].Xn1); b.st_next = R.st(last ? t->stDummy : t->sv[l + 1].st1);
        // last layer: optionally tap the concept tokens' attention rows over the patch tokens (attn_cache[-1][:, :, -Q:, 1:-Q])
        // (concept_attn_all_layers of the call: every layer's rows, [L, B, heads, Q, Np])
        float *cattn = !out_cattn_all ? nullptr
                       : t->attn_all_layers ? out_cattn_all + ((size_t)l * t->B + img0) * c.heads * Q * np
                       : last ? out_cattn_all + (size_t)img0 * c.heads * Q * np : nullptr;
        if (int e = ch_layer_forward(run, st, t->lw[l], b, cattn, t->prune_last && last ? Hc : nullptr)) return e;
    }
    H = st.H;   // the compact copy past a pruned last layer
    const int cur = st.cur;
    const int tok_out = cur == rows ? ntok : nq;   // row layout of the final residual: all tokens, or (CLS, concept tokens) per image
    if (int e = ch_gather_concept_rows(H, B, tok_out, Q, D, out_hf_all + (size_t)img0 * Q * D, s)) return e;
    if (out_cls_all) {  // CLS rows of the final residual (the pooled branch, models/arch/coop.py:484-499, is not part of the loss)
        CH_CHECK_HIP(hipMemcpy2DAsync(out_cls_all + (size_t)img0 * D, sizeof(float) * D, H, sizeof(float) * (size_t)tok_out * D, sizeof(float) * D, B,
                                      hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

int backward_chain(ch_trainer *t, int ch, const float *dhf_all, const float *dcattn_all, int img0, int B, hipStream_t s) {
    ch_model *m = t->m;
    const ch_model_config &c = m->cfg;
    const int D = c.dim, M = c.ffn, ntok = m->ntok, bpad = m->bpad, Q = c.ncontext, L = c.layers, b = c.adapter_dim, nq = 1 + Q;
    const int rows = B * ntok;
    const Rows R{t->row_off[ch], D, M, bpad};
    const float *zero = m->zero_bias;
    float *grads = ch == 0 ? t->grads : t->grads1;
    // trainable backbone: this chain's gradient arena, and the fp32 copy of d(branch input) the bias gradients are summed from (the
    // forward's residual buffer is free during backward)
    const bool bb = t->bb;
    float *bgrads = ch == 0 ? t->bgrads : t->bgrads1;
    float *dMf = bb ? R.d(t->H) : nullptr;
    bf16_t *dMb = R.d(t->dMb), *tD = R.d(t->tD), *tD2 = R.d(t->tD2), *tB = R.b(t->tB), *tM = R.m(t->tM), *tQKV = R.d3(t->tQKV);
    const int64_t ralloc = t->region_rows[ch];
    // gradient of the residual stream: fp32 + its bf16 copy.  Full token rows, or -- inside the pruned last layer -- the compact
    // (CLS, concept tokens) rows of every image
    float *dHfull = R.d(t->dH), *dHc = t->dHc + (size_t)ch * t->hc_rows * D;
    bf16_t *dHbfull = R.d(t->dHb), *dHcb = t->dHcb + (size_t)ch * t->hc_rows * D;
    const bool prune = t->prune_last;
    float *dH = prune ? dHc : dHfull;
    bf16_t *dHb = prune ? dHcb : dHbfull;
    int cur = prune ? B * nq : rows;
    // the loss reads only hash_features = H[:, -Q:, :] (models/arch/coop.py:484-486): dH is zero elsewhere
    if (int e = ch_scatter_concept_rows(dhf_all + (size_t)img0 * Q * D, B, prune ? nq : ntok, Q, D, dH, dHb, s)) return e;

    // gradient of the block output arrives in dH / dHb; leaves d(branch input) = dH + adapter path in dMb (bf16 only)
    auto adapter_bwd = [&](int l, int a) -> int {
        const AdWork &aw = t->ad[l * 2 + a];
        const Saved &v = t->sv[l];
        float *pbase = t->params + (int64_t)(l * 2 + a) * t->ad_numel;
        const AdPtr ap = ad_ptrs(pbase, c);
        const bf16_t *in = R.d(a == 0 ? v.A : v.A2), *P = R.b(a == 0 ? v.P1 : v.P2), *G = R.b(a == 0 ? v.G1 : v.G2);
        const float *stin = R.st(a == 0 ? v.stA : v.stA2);
        const int64_t dalloc = dHb == dHcb ? t->hc_rows : ralloc;
        // up projection: weight-gradient products (unscaled) and dgrad
        const bool bg = t->batched_grads;
        const int ai = l * 2 + a;
        int nchunk[4] = {0, 0, 0, 0};   // G, cu, T, cd
        if (int e = ch_wgrad_tn(dHb, D, G, bpad, cur, dalloc, D, bpad, t->G[ch], t->ws_wgrad[ch], s, bg ? &nchunk[0] : nullptr)) return e;
        // of the fp32 gradient: a bias gradient is a sum over rows that largely cancels, the bf16 copy costs 1e-1 relative there
        if (int e = ch_colsum(dH, 1, D, cur, D, t->cu[ch], t->ws_colsum[ch], s, bg ? &nchunk[1] : nullptr)) return e;
        ChGemmCall g{bpad, D, dHb, aw.up_wT, zero, EPI_BIAS_DACT_GELU};   // dpre = s (dH W_up) o gelu'(pre), in the epilogue
        g.out = tB; g.ldo = bpad; g.aux = P; g.scale = ap.scale;
        if (int e = gemm(t, ch, cur, g, s, dalloc)) return e;
        // down projection + adapter LayerNorm: the input-gradient GEMM and the LayerNorm backward first -- the latter emits the
        // normalised adapter input x_hat (bf16) on the way, which the weight-gradient product then consumes
        g = ChGemmCall{D, bpad, tB, aw.down_wgT, zero, EPI_BIAS};
        g.out = tD; g.ldo = D;
        if (int e = gemm(t, ch, cur, g, s)) return e;
        if (int e = ch_ln_bwd(tD, in, stin, cur, D, 1e-5f, dH, dMf, dMb, s, tD2)) return e;
        if (int e = ch_wgrad_tn(tB, bpad, tD2, D, cur, ralloc, bpad, D, t->T[ch], bg ? t->ws_wgradT[ch] : t->ws_wgrad[ch], s, bg ? &nchunk[2] : nullptr))
            return e;
        if (int e = ch_colsum(tB, 0, bpad, cur, bpad, t->cd[ch], bg ? t->ws_colsumD[ch] : t->ws_colsum[ch], s, bg ? &nchunk[3] : nullptr)) return e;
        if (bg) {
            const ChReduceJob jobs[4] = {{t->ws_wgrad[ch], t->Gs[ch] + (size_t)ai * D * bpad, nchunk[0], D * bpad / 4},
                                         {t->ws_colsum[ch], t->cus[ch] + (size_t)ai * D, nchunk[1], D / 4},
                                         {t->ws_wgradT[ch], t->Ts[ch] + (size_t)ai * bpad * D, nchunk[2], bpad * D / 4},
                                         {t->ws_colsumD[ch], t->cds[ch] + (size_t)ai * bpad, nchunk[3], bpad / 4}};
            return ch_reduce_partials_multi(jobs, 4, s);
        }
        return ch_adapter_grads(t->G[ch], t->cu[ch], t->T[ch], t->cd[ch], pbase, D, b, bpad, grads + (int64_t)(l * 2 + a) * t->ad_numel,
                                t->ws_colsum[ch], s);
    };

    // ---- trainable backbone: weight gradients from the operands the chain has in hand anyway (all of it behind `bb`)
    // plain Linear: dW [N, K] = dy^T x straight into the arena, db = fp32 column sums of dy (a cancelled sum: train.hip adapter_bwd)
    auto plain_grads = [&](bf16_t *dy_b, const float *dy_f, const bf16_t *xin, int N, int K, int64_t dyalloc, float *dW, float *db) -> int {
        if (int e = ch_wgrad_tn(dy_b, N, xin, K, cur, dyalloc, N, K, dW, t->ws_bb[ch], s)) return e;
        return ch_colsum(dy_f, 1, N, cur, N, db, t->ws_bbcol[ch], s);
    };
    // Linear with its input LayerNorm folded in: T = dpre^T x_hat, c = colsum(dpre), assembled by ch_fold_grads
    auto folded_grads = [&](bf16_t *dpre, const bf16_t *xhat, int N, const ChFoldGradParts &parts, const float *gamma, const float *beta,
                            float *dgamma, float *dbeta) -> int {
        if (int e = ch_wgrad_tn(dpre, N, xhat, D, cur, ralloc, N, D, t->Tbb[ch], t->ws_bb[ch], s)) return e;
        if (int e = ch_colsum(dpre, 0, N, cur, N, t->cbb[ch], t->ws_bbcol[ch], s)) return e;
        return ch_fold_grads(t->Tbb[ch], t->cbb[ch], gamma, beta, D, parts, dgamma, dbeta, s);
    };
    for (int l = L - 1; l >= 0; --l) {
        const Saved &v = t->sv[l];
        const LayerT &x = t->lt[l];
        const BbPtr bp = bb ? bb_ptrs(t->bparams + (int64_t)l * t->bb_layer_numel, c) : BbPtr{};
        const BbPtr bg = bb ? bb_ptrs(bgrads + (int64_t)l * t->bb_layer_numel, c) : BbPtr{};
        // ---- x_out = x_mid + m + adapter_2(m),  m = fc2(act(fc1(LN2(x_mid))))
        if (int e = adapter_bwd(l, 1)) return e;
        if (bb) {   // fc2: dM^T act(F1); act(F1) is recomputed from the saved pre-activation (no extra saved bytes)
            if (int e = ch_act_fwd(R.m(v.F1pre), (int64_t)cur * M, c.act == 0 ? 0 : 1, R.m(t->F1act), s)) return e;
            if (int e = plain_grads(dMb, dMf, R.m(t->F1act), D, M, ralloc, bg.fc2_w, bg.fc2_b)) return e;
        }
        ChGemmCall g{M, D, dMb, x.fc2_wT, zero, c.act == 0 ? EPI_BIAS_DACT_QUICK : EPI_BIAS_DACT_GELU};
        g.out = tM; g.ldo = M; g.aux = R.m(v.F1pre);
        if (int e = gemm(t, ch, cur, g, s)) return e;
        g = ChGemmCall{D, M, tM, x.fc1_wgT, zero, EPI_BIAS};
        g.out = tD; g.ldo = D;
        if (int e = gemm(t, ch, cur, g, s)) return e;
        if (int e = ch_ln_bwd(tD, R.d(v.Xn2), R.st(v.st2), cur, D, c.ln_eps, dH, dH, dHb, s, bb ? tD2 : nullptr)) return e;
        if (bb) {   // fc1 with layer_norm2 folded: tM^T x_hat_2
            ChFoldGradParts parts{{bp.fc1_w, nullptr, nullptr}, {bg.fc1_w, nullptr, nullptr}, {bg.fc1_b, nullptr, nullptr}, 1, M};
            if (int e = folded_grads(tM, tD2, M, parts, bp.ln2_w, bp.ln2_b, bg.ln2_w, bg.ln2_b)) return e;
        }
        // ---- x_mid = x_in + a + adapter_1(a),  a = out_proj(attention(qkv(LN1(x_in))))
        if (int e = adapter_bwd(l, 0)) return e;
        if (bb)     // out_proj: dA^T ctx (the saved attention output; compact rows inside the pruned last layer, as dA is)
            if (int e = plain_grads(dMb, dMf, R.d(v.AO), D, D, ralloc, bg.out_w, bg.out_b)) return e;
        g = ChGemmCall{D, D, dMb, x.out_wT, zero, EPI_BIAS};
        g.out = tD; g.ldo = D;
        if (int e = gemm(t, ch, cur, g, s)) return e;
        const bf16_t *dctx = tD;
        if (cur != rows) {
            // leaving the pruned part of the last layer: the compact gradients go back to their token rows (zeros elsewhere) --
            // attention's keys / values cover every token, so from here on all rows carry gradient
            if (int e = ch_expand_head_rows(tD, 0, B, ntok, Q, D, tD2, s)) return e;
            if (int e = ch_expand_head_rows(dH, 1, B, ntok, Q, D, dHfull, s)) return e;
            dctx = tD2;
            dH = dHfull;
            dHb = dHbfull;
            cur = rows;
        }
        const float *dpext = !dcattn_all ? nullptr
                             : t->attn_all_layers ? dcattn_all + ((size_t)l * t->B + img0) * c.heads * Q * (ntok - Q - 1)
                             : l == L - 1 ? dcattn_all + (size_t)img0 * c.heads * Q * (ntok - Q - 1) : nullptr;
        if (int e = ch_attention_bwd(R.d3(v.QKV), dctx, B, ntok, c.heads, tQKV, s, dpext, Q, m->attn_stream ? 2 : 0)) return e;
        g = ChGemmCall{D, 3 * D, tQKV, x.qkv_wgT, zero, EPI_BIAS};
        g.out = tD; g.ldo = D;
        if (int e = gemm(t, ch, cur, g, s)) return e;
        if (int e = ch_ln_bwd(tD, R.d(v.Xn1), R.st(v.st1), cur, D, c.ln_eps, dH, dH, dHb, s, bb ? tD2 : nullptr)) return e;
        if (bb) {   // q | k | v with layer_norm1 folded: tQKV^T x_hat_1
            ChFoldGradParts parts{{bp.qkv_w[0], bp.qkv_w[1], bp.qkv_w[2]}, {bg.qkv_w[0], bg.qkv_w[1], bg.qkv_w[2]},
                                  {bg.qkv_b[0], bg.qkv_b[1], bg.qkv_b[2]}, 3, D};
            if (int e = folded_grads(tQKV, tD2, 3 * D, parts, bp.ln1_w, bp.ln1_b, bg.ln1_w, bg.ln1_b)) return e;
        }
    }
    if (t->batched_grads)   // every adapter's reduced products are in their slots: one launch pair assembles all the gradients
        if (int e = ch_adapter_grads(t->Gs[ch], t->cus[ch], t->Ts[ch], t->cds[ch], t->params, D, b, bpad, grads, t->ws_ag[ch], s, 2 * L, t->ad_numel))
            return e;
    // ---- concept tokens: rows ntok-Q.. of every image are pre_layrnorm(ctx[q]) (models/arch/coop.py:470-472)
    if (int e = ch_concept_rows_sum(dH, B, ntok, Q, D, t->dctx_sum[ch], s)) return e;
    if (!bb) return 0;
    // ---- trainable backbone, embedding side (models/arch/coop.py:452-472).  dH is the gradient of pre_layrnorm's output on every row.
    const int np = m->np, Kp = m->Kp, K = 3 * c.patch * c.patch;
    const BbEmb eg = bb_emb_ptrs(bgrads, c);
    if (int e = ch_colsum(dH, 1, D, rows, D, eg.pre_b, t->ws_bbcol[ch], s)) return e;
    // the pre-LayerNorm input is not kept (the forward normalises in place): its patch rows are the patch GEMM once more, on the im2col
    // matrix the forward left in PATCH
    float *X = R.d(t->H);
    bf16_t *PATCH = t->PATCH + t->prow_off[ch] * Kp;
    {
        GemmParams p{};
        p.X = PATCH; p.W = t->patch_w; p.M = B * np; p.N = D; p.K = Kp; p.X_rows_alloc = t->region_prows[ch];
        p.resid = X; p.ldr = D; p.pos = t->pos; p.tokens_per_img = ntok; p.patches_per_img = np; p.pp_min_k = m->pp_min_k;
        if (int e = ch_gemm_bf16(p, EPI_PATCH, s)) return e;
    }
    if (int e = ch_embed_bwd(X, dH, B, ntok, np, D, t->cls_pos0, t->ctx, t->pre_w, c.ln_eps, tD, s)) return e;
    if (int e = ch_colsum(X, 1, D, rows, D, eg.pre_w, t->ws_bbcol[ch], s)) return e;
    // position table (the table the forward added: rows 0 .. np); the class embedding enters row 0 only
    if (int e = ch_token_rows_sum(dH, B, ntok, np + 1, D, eg.pos, s)) return e;
    CH_CHECK_HIP(hipMemcpyAsync(eg.cls, eg.pos, sizeof(float) * D, hipMemcpyDeviceToDevice, s));
    // patch weight: (patch rows of dx)^T im2col -> [D, Kp], of which the first K columns are the parameter's
    if (int e = ch_wgrad_tn(tD, D, PATCH, Kp, (int64_t)B * np, std::min(ralloc, t->region_prows[ch]), D, Kp, t->Tbb[ch], t->ws_bb[ch], s)) return e;
    CH_CHECK_HIP(hipMemcpy2DAsync(eg.patch_w, sizeof(float) * K, t->Tbb[ch], sizeof(float) * Kp, sizeof(float) * K, D, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // namespace

extern "C" int64_t ch_adapter_arena_numel(const ch_model *m) {
    if (!m || m->cfg.adapter_dim <= 0) return 0;
    return adapter_numel(m->cfg) * m->cfg.layers * 2;
}

extern "C" void ch_trainer_destroy(ch_trainer *t) {
    delete t;
}

extern "C" int ch_trainer_refresh(ch_trainer *t, void *stream) {
    CH_REQUIRE(t != nullptr, "null trainer");
    const ch_model_config &c = t->m->cfg;
    const AdWork &w = t->ad[0];   // slot 0 of the contiguous per-field arrays
    hipStream_t s = (hipStream_t)stream;
    if (int e = ch_adapter_refresh(t->params, t->ad_numel, c.layers * 2, c.dim, c.adapter_dim, t->m->bpad, w.down_wf, w.fold_c, w.fold_d, w.up_w,
                                   w.up_wT, w.down_wgT, s))
        return e;
    if (!t->bb) return 0;
    // trainable backbone: bf16 / LayerNorm-folded copies for the forward, (W o gamma)^T and W^T for the input-gradient GEMMs
    const int D = c.dim, M = c.ffn, K = 3 * c.patch * c.patch;
    for (int l = 0; l < c.layers; ++l) {
        const BbPtr p = bb_ptrs(t->bparams + (int64_t)l * t->bb_layer_numel, c);
        const BbWork &b = t->bw[l];
        const LayerT &x = t->lt[l];
        for (int j = 0; j < 3; ++j) {
            if (int e = ch_fold_ln(p.qkv_w[j], p.qkv_b[j], p.ln1_w, p.ln1_b, D, D, D, b.qkv_wf + (size_t)j * D * D, b.qkv_c + j * D, b.qkv_d + j * D, s))
                return e;
            if (int e = ch_transpose_f32_to_bf16(p.qkv_w[j], D, D, D, p.ln1_w, x.qkv_wgT + j * D, 3 * D, s)) return e;
        }
        if (int e = ch_fold_ln(p.fc1_w, p.fc1_b, p.ln2_w, p.ln2_b, M, M, D, b.fc1_wf, b.fc1_c, b.fc1_d, s)) return e;
        if (int e = ch_transpose_f32_to_bf16(p.fc1_w, M, D, D, p.ln2_w, x.fc1_wgT, M, s)) return e;
        if (int e = ch_convert_bf16(p.out_w, D, D, D, b.out_w, s)) return e;
        if (int e = ch_transpose_f32_to_bf16(p.out_w, D, D, D, nullptr, x.out_wT, D, s)) return e;
        if (int e = ch_convert_bf16(p.fc2_w, D, M, M, b.fc2_w, s)) return e;
        if (int e = ch_transpose_f32_to_bf16(p.fc2_w, D, M, M, nullptr, x.fc2_wT, D, s)) return e;
    }
    const BbEmb e = bb_emb_ptrs(t->bparams, c);
    if (int r = ch_convert_bf16(e.patch_w, D, K, t->m->Kp, t->bb_patch_w, s)) return r;
    return ch_small_add(e.cls, e.pos, D, t->bb_cls_pos0, s);
}

extern "C" int64_t ch_backbone_arena_numel(const ch_model_config *cfg) {
    if (!cfg || cfg->dim <= 0 || cfg->patch <= 0 || cfg->layers <= 0) return 0;
    return bb_layer_numel(*cfg) * cfg->layers + bb_emb_numel(*cfg);
}

// name: a state-dict key below `vision_model.` ("encoder.layers.3.self_attn.q_proj.weight", "embeddings.class_embedding", ...)
extern "C" int64_t ch_backbone_arena_offset(const ch_model_config *cfg, const char *name, int64_t *numel) {
    if (!cfg || !name || cfg->dim <= 0 || cfg->patch <= 0 || cfg->layers <= 0) return -1;
    const ch_model_config &c = *cfg;
    const int64_t D = c.dim, M = c.ffn;
    const std::string n(name);
    int64_t off = -1, cnt = 0;
    const std::string lp = "encoder.layers.";
    if (n.compare(0, lp.size(), lp) == 0) {
        const size_t dot = n.find('.', lp.size());
        if (dot == std::string::npos || dot == lp.size()) return -1;
        int64_t l = 0;
        for (size_t i = lp.size(); i < dot; ++i) {
            if (n[i] < '0' || n[i] > '9' || l > c.layers) return -1;
            l = l * 10 + (n[i] - '0');
        }
        if (l >= c.layers) return -1;
        const std::string f = n.substr(dot + 1);
        static const char *names[16] = {"layer_norm1.weight", "layer_norm1.bias", "self_attn.q_proj.weight", "self_attn.q_proj.bias",
                                        "self_attn.k_proj.weight", "self_attn.k_proj.bias", "self_attn.v_proj.weight", "self_attn.v_proj.bias",
                                        "self_attn.out_proj.weight", "self_attn.out_proj.bias", "layer_norm2.weight", "layer_norm2.bias",
                                        "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"};
        const int64_t sizes[16] = {D, D, D * D, D, D * D, D, D * D, D, D * D, D, D, D, M * D, M, D * M, D};
        int64_t o = l * bb_layer_numel(c);
        for (int i = 0; i < 16; ++i) {
            if (f == names[i]) {
                off = o;
                cnt = sizes[i];
                break;
            }
            o += sizes[i];
        }
    } else {
        const int64_t g = c.image_size / c.patch;
        static const char *names[5] = {"embeddings.class_embedding", "embeddings.patch_embedding.weight", "embeddings.position_embedding.weight",
                                       "pre_layrnorm.weight", "pre_layrnorm.bias"};
        const int64_t sizes[5] = {D, D * 3 * c.patch * c.patch, (g * g + 1) * D, D, D};
        int64_t o = bb_layer_numel(c) * c.layers;
        for (int i = 0; i < 5; ++i) {
            if (n == names[i]) {
                off = o;
                cnt = sizes[i];
                break;
            }
            o += sizes[i];
        }
    }
    if (off >= 0 && numel) *numel = cnt;
    return off;
}

extern "C" int ch_trainer_create(ch_model *m, int32_t max_batch, float *params, float *grads, ch_trainer **out) {
    return ch_trainer_create_ex(m, max_batch, params, grads, nullptr, nullptr, out);
}

extern "C" int ch_trainer_create_ex(ch_model *m, int32_t max_batch, float *params, float *grads, float *backbone_params, float *backbone_grads,
                                    ch_trainer **out) {
    CH_REQUIRE(out != nullptr, "null out pointer");
    *out = nullptr;
    CH_REQUIRE(m != nullptr && params != nullptr && grads != nullptr, "trainer: null model / parameter arena / gradient arena");
    CH_REQUIRE((backbone_params == nullptr) == (backbone_grads == nullptr), "trainer: the backbone arenas come as a pair (both or neither)");
    const ch_model_config &c = m->cfg;
    CH_REQUIRE(backbone_params == nullptr || (m->Kp % 128 == 0 && c.ffn % 128 == 0 && c.dim % 128 == 0),
               "trainer: a trainable backbone needs dim, ffn and the padded patch length 3*patch^2 to be multiples of 128");
    CH_REQUIRE(c.adapter_dim > 0, "trainer: the model has no adapters (nothing to train in the encoder)");
    CH_REQUIRE(max_batch >= 1, "trainer: max_batch must be >= 1");
    CH_REQUIRE(m->layers[0].qkv_wf != nullptr, "trainer: the model was built without the LayerNorm-folded weights");
    ch_trainer *t = new ch_trainer();
    t->m = m;
    t->max_batch = max_batch;
    t->params = params;
    t->grads = grads;
    t->ad_numel = adapter_numel(c);
    t->bb = backbone_params != nullptr;
    t->bparams = backbone_params;
    t->bgrads = backbone_grads;
    t->bb_layer_numel = bb_layer_numel(c);
    t->bb_numel = t->bb_layer_numel * c.layers + bb_emb_numel(c);
    t->lw = m->layers;
    t->patch_w = m->patch_w; t->pos = m->pos; t->cls_pos0 = m->cls_pos0; t->pre_w = m->pre_w; t->pre_b = m->pre_b;
    // options of the model the trainer is created on (ch_model_set_option "train_chains" / "train_chain_min_rows" / "train_prune_last")
    t->nchains = std::max(1, std::min(m->train_chains, TR_CHAINS));
    t->chain_min_rows = std::max<int64_t>(0, m->train_chain_min_rows);
    t->prune_last = m->train_prune_last;
    t->batched_grads = m->train_batched_grads;
    const int D = c.dim, L = c.layers, M = c.ffn, bpad = m->bpad, Q = c.ncontext;
    // region 0 holds a whole batch (one chain) or the first half (two chains); region 1 the second half
    const int half = (max_batch + 1) / 2;
    t->region_rows[0] = round_up64((int64_t)max_batch * m->ntok, 256) + 256;
    t->region_prows[0] = round_up64((int64_t)max_batch * m->np, 256) + 256;
    t->region_rows[1] = t->nchains > 1 ? round_up64((int64_t)half * m->ntok, 256) + 256 : 0;
    t->region_prows[1] = t->nchains > 1 ? round_up64((int64_t)half * m->np, 256) + 256 : 0;
    t->row_off[1] = t->region_rows[0];
    t->prow_off[1] = t->region_prows[0];
    const int64_t rows = t->region_rows[0] + t->region_rows[1], prows = t->region_prows[0] + t->region_prows[1];
    bool ok = true;
    if (t->nchains > 1 && !t->fj.init(t->own, 2)) {
        ch_set_error("trainer: cannot create the auxiliary stream / events");
        ok = false;
    }
    auto bf = [&](int64_t cols) { return (bf16_t *)talloc(t, sizeof(bf16_t) * rows * cols, ok); };
    auto st = [&]() { return (float *)talloc(t, sizeof(float) * rows * (D / 64) * 2, ok); };
    t->ad.resize(L * 2);
    t->lt.resize(L);
    t->sv.resize(L);
    {   // one contiguous array per field, one slot per adapter (ch_adapter_refresh fills all slots in one launch per field);
        // zero-initialised: the padding rows / columns (bottleneck b -> bpad) are never written again
        const size_t nad = (size_t)L * 2, mat = (size_t)bpad * D;
        bf16_t *dwf = (bf16_t *)talloc(t, sizeof(bf16_t) * nad * mat, ok), *uw = (bf16_t *)talloc(t, sizeof(bf16_t) * nad * mat, ok),
               *uwT = (bf16_t *)talloc(t, sizeof(bf16_t) * nad * mat, ok), *dwT = (bf16_t *)talloc(t, sizeof(bf16_t) * nad * mat, ok);
        float *fc = (float *)talloc(t, sizeof(float) * nad * bpad, ok), *fd = (float *)talloc(t, sizeof(float) * nad * bpad, ok);
        for (size_t i = 0; i < nad && ok; ++i) {
            AdWork &w = t->ad[i];
            w.down_wf = dwf + i * mat; w.up_w = uw + i * mat; w.up_wT = uwT + i * mat; w.down_wgT = dwT + i * mat;
            w.fold_c = fc + i * bpad; w.fold_d = fd + i * bpad;
            // what the forward reads (layer_forward.h): these working copies; bias and scale straight from the parameter arena
            AdapterW &fw = t->lw[i / 2].ad[i % 2];
            const AdPtr ap = ad_ptrs(t->params + (int64_t)i * t->ad_numel, c);
            fw.down_wf = w.down_wf; fw.fold_c = w.fold_c; fw.fold_d = w.fold_d; fw.up_w = w.up_w; fw.up_b = ap.up_b; fw.scale = ap.scale;
        }
    }
    hipStream_t s = nullptr;
    for (int l = 0; l < L && ok; ++l) {
        const LayerW &w = m->layers[l];
        LayerT &x = t->lt[l];
        x.qkv_wgT = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)D * 3 * D, ok);
        x.out_wT = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)D * D, ok);
        x.fc1_wgT = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)D * M, ok);
        x.fc2_wT = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)M * D, ok);
        if (!ok) break;
        if (!t->bb) {
            // the folded weights already carry gamma: W' = bf16(W * gamma) [N, D] -> (W')^T [D, N]
            int e = ch_transpose_bf16(w.qkv_wf, 3 * D, D, D, x.qkv_wgT, 3 * D, s);
            e |= ch_transpose_bf16(w.out_w, D, D, D, x.out_wT, D, s);
            e |= ch_transpose_bf16(w.fc1_wf, M, D, D, x.fc1_wgT, M, s);
            e |= ch_transpose_bf16(w.fc2_w, D, M, M, x.fc2_wT, D, s);
            if (e) ok = false;
        }
        Saved &v = t->sv[l];
        v.Xn1 = bf(D); v.QKV = bf(3 * D); v.AO = bf(D); v.A = bf(D); v.P1 = bf(bpad); v.G1 = bf(bpad); v.Xn2 = bf(D);
        v.F1pre = bf(M); v.A2 = bf(D); v.P2 = bf(bpad); v.G2 = bf(bpad);
        v.st1 = st(); v.stA = st(); v.st2 = st(); v.stA2 = st();
    }
    t->H = (float *)talloc(t, sizeof(float) * rows * D, ok);
    t->dH = (float *)talloc(t, sizeof(float) * rows * D, ok);
    t->dHb = bf(D); t->dMb = bf(D); t->tD = bf(D); t->tD2 = bf(D); t->tB = bf(bpad); t->tM = bf(M); t->tQKV = bf(3 * D); t->F1act = bf(M);
    t->XnDummy = bf(D);
    t->stDummy = st();
    t->PATCH = (bf16_t *)talloc(t, sizeof(bf16_t) * prows * m->Kp, ok);
    t->ctx = (float *)talloc(t, sizeof(float) * Q * D, ok);
    t->hc_rows = round_up64((int64_t)max_batch * (1 + Q), 256) + 256;
    t->Hc = (float *)talloc(t, sizeof(float) * t->hc_rows * TR_CHAINS * D, ok);
    t->dHc = (float *)talloc(t, sizeof(float) * t->hc_rows * TR_CHAINS * D, ok);
    t->dHcb = (bf16_t *)talloc(t, sizeof(bf16_t) * t->hc_rows * TR_CHAINS * D, ok);
    const int64_t max_rows = (int64_t)max_batch * m->ntok;
    for (int ch = 0; ch < t->nchains; ++ch) {
        t->ws_wgrad[ch] = (float *)talloc(t, sizeof(float) * std::max(ch_wgrad_ws_floats(max_rows, D, bpad), ch_wgrad_ws_floats(max_rows, bpad, D)), ok);
        t->ws_colsum[ch] = (float *)talloc(t, sizeof(float) * ch_colsum_ws_floats(std::max(D, bpad)), ok);
        if (t->batched_grads) {
            const size_t nad = (size_t)L * 2;
            t->ws_wgradT[ch] = (float *)talloc(t, sizeof(float) * std::max(ch_wgrad_ws_floats(max_rows, D, bpad), ch_wgrad_ws_floats(max_rows, bpad, D)), ok);
            t->ws_colsumD[ch] = (float *)talloc(t, sizeof(float) * ch_colsum_ws_floats(std::max(D, bpad)), ok);
            t->Gs[ch] = (float *)talloc(t, sizeof(float) * nad * D * bpad, ok);
            t->Ts[ch] = (float *)talloc(t, sizeof(float) * nad * bpad * D, ok);
            t->cus[ch] = (float *)talloc(t, sizeof(float) * nad * D, ok);
            t->cds[ch] = (float *)talloc(t, sizeof(float) * nad * bpad, ok);
            t->ws_ag[ch] = (float *)talloc(t, sizeof(float) * ch_adapter_grads_ws_floats(nad), ok);
        }
        t->G[ch] = (float *)talloc(t, sizeof(float) * (size_t)D * bpad, ok);
        t->T[ch] = (float *)talloc(t, sizeof(float) * (size_t)bpad * D, ok);
        t->cu[ch] = (float *)talloc(t, sizeof(float) * D, ok);
        t->cd[ch] = (float *)talloc(t, sizeof(float) * bpad, ok);
        t->dctx_sum[ch] = (float *)talloc(t, sizeof(float) * Q * D, ok);
    }
    if (t->nchains > 1) t->grads1 = (float *)talloc(t, sizeof(float) * t->ad_numel * L * 2, ok);
    if (t->bb) {   // working copies (filled by ch_trainer_refresh below), weight-gradient scratch, the second chain's gradient arena
        t->bw.resize(L);
        for (int l = 0; l < L; ++l) {
            BbWork &b = t->bw[l];
            b.qkv_wf = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)3 * D * D, ok);
            b.out_w = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)D * D, ok);
            b.fc1_wf = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)M * D, ok);
            b.fc2_w = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)D * M, ok);
            b.qkv_c = (float *)talloc(t, sizeof(float) * 3 * D, ok);
            b.qkv_d = (float *)talloc(t, sizeof(float) * 3 * D, ok);
            b.fc1_c = (float *)talloc(t, sizeof(float) * M, ok);
            b.fc1_d = (float *)talloc(t, sizeof(float) * M, ok);
            if (!ok) break;
            const BbPtr p = bb_ptrs(t->bparams + (int64_t)l * t->bb_layer_numel, c);
            LayerW &w = t->lw[l];
            w.ln1_w = p.ln1_w; w.ln1_b = p.ln1_b; w.ln2_w = p.ln2_w; w.ln2_b = p.ln2_b;
            w.qkv_w = nullptr; w.fc1_w = nullptr; w.qkv_b = nullptr; w.fc1_b = nullptr;      // the folded forms are what the chain reads
            w.qkv_wf = b.qkv_wf; w.qkv_c = b.qkv_c; w.qkv_d = b.qkv_d; w.out_w = b.out_w; w.out_b = p.out_b;
            w.fc1_wf = b.fc1_wf; w.fc1_c = b.fc1_c; w.fc1_d = b.fc1_d; w.fc2_w = b.fc2_w; w.fc2_b = p.fc2_b;
        }
        t->bb_patch_w = (bf16_t *)talloc(t, sizeof(bf16_t) * (size_t)D * m->Kp, ok);
        t->bb_cls_pos0 = (float *)talloc(t, sizeof(float) * D, ok);
        const BbEmb e = bb_emb_ptrs(t->bparams, c);
        t->patch_w = t->bb_patch_w; t->pos = e.pos; t->cls_pos0 = t->bb_cls_pos0; t->pre_w = e.pre_w; t->pre_b = e.pre_b;
        const int Kp = m->Kp;
        const size_t wsf = std::max({ch_wgrad_ws_floats(max_rows, D, M), ch_wgrad_ws_floats(max_rows, M, D), ch_wgrad_ws_floats(max_rows, 3 * D, D),
                                     ch_wgrad_ws_floats(max_rows, D, D), ch_wgrad_ws_floats(max_rows, D, Kp)});
        for (int ch = 0; ch < t->nchains; ++ch) {
            t->ws_bb[ch] = (float *)talloc(t, sizeof(float) * wsf, ok);
            t->ws_bbcol[ch] = (float *)talloc(t, sizeof(float) * ch_colsum_ws_floats(std::max(3 * D, M)), ok);
            t->Tbb[ch] = (float *)talloc(t, sizeof(float) * (size_t)D * std::max({3 * D, M, Kp}), ok);
            t->cbb[ch] = (float *)talloc(t, sizeof(float) * std::max(3 * D, M), ok);
        }
        if (t->nchains > 1) t->bgrads1 = (float *)talloc(t, sizeof(float) * t->bb_numel, ok);
    }
    if (ok && ch_trainer_refresh(t, nullptr) != 0) ok = false;
    if (ok && hipDeviceSynchronize() != hipSuccess) {
        ch_set_error("trainer: device error while preparing the working copies");
        ok = false;
    }
    if (!ok) {
        ch_trainer_destroy(t);
        return 4;
    }
    *out = t;
    return 0;
}

extern "C" int64_t ch_trainer_bytes(const ch_trainer *t) { return t ? (int64_t)t->own.bytes() : 0; }

extern "C" int ch_train_forward(ch_trainer *t, const void *images, int32_t image_dtype, int32_t B, const float *concept_tokens,
                                float *out_hash_features, float *out_cls, float *out_concept_attn, int32_t concept_attn_all_layers,
                                void *stream) {
    CH_REQUIRE(t != nullptr && images != nullptr && concept_tokens != nullptr && out_hash_features != nullptr, "train_forward: null argument");
    CH_REQUIRE(B >= 1 && B <= t->max_batch, "train_forward: batch outside [1, max_batch]");
    CH_REQUIRE(image_dtype == 0 || image_dtype == 1, "train_forward: image_dtype must be 0 (fp32) or 1 (bf16)");
    hipStream_t s = (hipStream_t)stream;
    const ch_model_config &c = t->m->cfg;
    t->B = B;
    t->forward_done = false;
    t->attn_all_layers = out_concept_attn != nullptr && concept_attn_all_layers != 0;
    CH_CHECK_HIP(hipMemcpyAsync(t->ctx, concept_tokens, sizeof(float) * c.ncontext * c.dim, hipMemcpyDeviceToDevice, s));
    {
        // Two micro-batch chains or one?  Option "train_chain_min_rows" > 0: two when each chain has at least that many token rows.  0 (default):
        // two when ONE chain's narrowest 256x256-tile GEMM (N = D: out_proj, fc2 and the input-gradient products) would need more than one
        // round of the chip's 256 CUs -- a second round that is nearly empty is what a single chain pays just above the boundary (batch 112
        // of ViT-B/16: 264 tiles, 18.4 ms against 16.5 with two chains; batch 96: 228 tiles, 14.3 against 15.5; profiles/r04_train_ab_two_chains.txt)
        const int64_t rows = (int64_t)B * t->m->ntok;
        const bool two = t->chain_min_rows > 0 ? (int64_t)(B / 2) * t->m->ntok >= t->chain_min_rows
                                               : ((rows + 255) / 256) * ((c.dim + 255) / 256) > 256;
        t->nc = (t->nchains > 1 && B >= 2 && two) ? 2 : 1;
    }
    if (t->nc == 1) {
        t->Bc[0] = B; t->Bc[1] = 0;
        if (int e = forward_chain(t, 0, images, image_dtype, 0, B, out_hash_features, out_cls, out_concept_attn, s)) return e;
    } else {
        t->Bc[0] = B - B / 2; t->Bc[1] = B / 2;      // chain 1 <= ceil(max_batch / 2) images: fits its region
        if (int e = t->fj.fork(s)) return e;
        if (int e = t->fj.start(1)) return e;
        if (int e = forward_chain(t, 0, images, image_dtype, 0, t->Bc[0], out_hash_features, out_cls, out_concept_attn, s)) return e;
        if (int e = forward_chain(t, 1, images, image_dtype, t->Bc[0], t->Bc[1], out_hash_features, out_cls, out_concept_attn, t->fj.aux[1])) return e;
        if (int e = t->fj.finish(1, s)) return e;
    }
    t->forward_done = true;
    return 0;
}

extern "C" int ch_train_backward(ch_trainer *t, const float *d_hash_features, const float *d_concept_attn, float *d_concept_tokens,
                                 void *stream) {
    CH_REQUIRE(t != nullptr && d_hash_features != nullptr && d_concept_tokens != nullptr, "train_backward: null argument");
    CH_REQUIRE(t->forward_done, "train_backward: call ch_train_forward first (its saved activations are what backward reads)");
    hipStream_t s = (hipStream_t)stream;
    const ch_model_config &c = t->m->cfg;
    const int Q = c.ncontext, D = c.dim;
    if (t->nc == 1) {
        if (int e = backward_chain(t, 0, d_hash_features, d_concept_attn, 0, t->Bc[0], s)) return e;
    } else {
        if (int e = t->fj.fork(s)) return e;
        if (int e = t->fj.start(1)) return e;
        if (int e = backward_chain(t, 0, d_hash_features, d_concept_attn, 0, t->Bc[0], s)) return e;
        if (int e = backward_chain(t, 1, d_hash_features, d_concept_attn, t->Bc[0], t->Bc[1], t->fj.aux[1])) return e;
        if (int e = t->fj.finish(1, s)) return e;
        // the two chains' contributions: parameter gradients and concept-token rows (both linear in the per-row products)
        if (int e = ch_small_add(t->grads, t->grads1, t->ad_numel * c.layers * 2, t->grads, s)) return e;
        if (t->bb)
            if (int e = ch_small_add(t->bgrads, t->bgrads1, t->bb_numel, t->bgrads, s)) return e;
        if (int e = ch_small_add(t->dctx_sum[0], t->dctx_sum[1], (int64_t)Q * D, t->dctx_sum[0], s)) return e;
    }
    return ch_small_ln_bwd(t->dctx_sum[0], t->ctx, t->pre_w, Q, D, c.ln_eps, d_concept_tokens, s);
}

// torch.optim.SGD semantics (maximize False) over a flat fp32 array, e.g. the adapter arena: see include/concepthash_hip.h
extern "C" int ch_sgd_step(float *params, const float *grads, float *momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                           float dampening, int32_t nesterov, int32_t first_step, void *stream) {
    CH_REQUIRE(params && grads && (momentum == 0.f || momentum_buf), "sgd_step: null argument");
    CH_REQUIRE(n > 0, "sgd_step: empty array");
    return ch_sgd_step_launch(params, grads, momentum_buf, n, lr, momentum, weight_decay, dampening, nesterov, first_step, (hipStream_t)stream);
}

// torch.optim.Adam / AdamW semantics (amsgrad False, maximize False) over a flat fp32 array: see include/concepthash_hip.h
extern "C" int ch_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                            double eps, double weight_decay, int32_t decoupled, int64_t step, void *stream) {
    CH_REQUIRE(params && grads && exp_avg && exp_avg_sq, "adam_step: null argument");
    CH_REQUIRE(n > 0 && step >= 1, "adam_step: empty array, or step < 1 (the first step is 1)");
    return ch_adam_step_launch(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, (hipStream_t)stream);
}
