// The forward pass of one encoder layer with folded LayerNorms: THE definition of its ten launches,
// qkv -> attention -> out_proj -> adapter down / up -> fc1 -> fc2 -> adapter down / up.  ch_encode (model.hip run_chain) and the
// training step (train.hip forward_chain) both issue it through ch_layer_forward; they differ only in the buffers they hand in
// (ChLayerBufs) and in the launcher object that turns a call into a launch.  Plain C++: tests/layer_forward_test.cpp records the
// sequence on the CPU.
#pragma once
#include "../../include/concepthash_hip.h"
#include "layer_types.h"

// One GEMM of a launch chain; each caller has one function that makes GemmParams of it with the options it forwards.
struct ChGemmCall {
    int N, K;
    const bf16_t *X, *W;
    const float *bias;
    int epi;
    bf16_t *out = nullptr;
    int ldo = 0;
    float *resid = nullptr;
    const float *scale = nullptr;
    const bf16_t *addend = nullptr;
    const float *stats_in = nullptr, *fold_c = nullptr;   // LayerNorm fold: statistics consumed ...
    float eps = 0.f;
    float *stats_out = nullptr;                           // ... and produced
    bf16_t *hb_out = nullptr;
    int ld_hb = 0;              // 0 = D
    const bf16_t *aux = nullptr;
    int cat = 0, n_true = 0, k_true = 0;   // profiler category; un-padded extents for the FLOP count (0 = N / K)
};

// This layer's buffers.  A null pre-activation buffer selects the one-output activation epilogue, null Xn_next / st_next the
// up-projection without statistics (nothing follows the chain's last layer).
struct ChLayerBufs {
    const bf16_t *Xn1;      // qkv input: bf16(H) with its row statistics st1 (qkv_folded), or rows already normalised by layer_norm1
    const float *st1;
    bool qkv_folded;
    bf16_t *QKV, *AO;       // qkv output, attention output
    bf16_t *A, *A2;         // out_proj / fc2 output (may be one buffer) ...
    float *stA, *stA2;      // ... and its row statistics
    bf16_t *AD[2];          // adapter activation (operand of the up-projection)
    bf16_t *ADpre[2];       // adapter pre-activation, or null
    bf16_t *Xn2;            // fc1 input: bf16(H) after the first adapter, statistics st2
    float *st2;
    bf16_t *F1, *F1pre;     // fc1 activation (operand of fc2); fc1 pre-activation, or null
    bf16_t *Xn_next;        // bf16(H) after the second adapter with its statistics: the next layer's Xn1 / st1, or null
    float *st_next;
};

struct ChChain {
    int B, ntok, Q, D, M, bpad, adapter_dim, act;   // act: 0 quick_gelu, 1 gelu (erf)
    float ln_eps;
    int cur;        // rows the GEMMs work on: all B * ntok token rows, or B * (1 + Q) once the last layer has pruned
    float *H;       // their fp32 residual stream
};

// adapter on the sub-block output `in` (statistics st_in): H += in + scale * up(gelu(down(LN(in)))), LN folded into the down-projection;
// xn_out / st_out (or null): bf16 copy of the updated H and its row statistics
template <class Launcher>
int ch_adapter_forward(Launcher &run, const ChChain &c, const AdapterW &aw, const bf16_t *in, const float *st_in, bf16_t *AD, bf16_t *ADpre,
                       bf16_t *xn_out, float *st_out) {
    ChGemmCall g{c.bpad, c.D, in, aw.down_wf, aw.fold_d, ADpre ? EPI_FOLD_ACT2_GELU : EPI_FOLD_GELU};
    g.cat = CH_CAT_GEMM_DOWN; g.n_true = c.adapter_dim;
    g.stats_in = st_in; g.fold_c = aw.fold_c; g.eps = 1e-5f; g.out = ADpre ? ADpre : AD; g.ldo = c.bpad;
    if (ADpre) { g.hb_out = AD; g.ld_hb = c.bpad; }   // the pre-activation is kept (backward), its GELU is the second output
    if (int e = run.gemm(c.cur, g)) return e;
    g = ChGemmCall{c.D, c.bpad, AD, aw.up_w, aw.up_b, st_out ? EPI_SCALE_RESID_STATS : EPI_SCALE_RESID};
    g.cat = CH_CAT_GEMM_UP; g.k_true = c.adapter_dim;
    g.resid = c.H; g.scale = aw.scale; g.addend = in; g.stats_out = st_out; g.hb_out = xn_out;
    return run.gemm(c.cur, g);
}

// Launcher: gemm(rows, ChGemmCall), attention(qkv, out, cattn, compact), gather_head_rows(H, Hc); each returns 0 or an error code.
// prune_into (the chain's last layer, or null): past the attention only CLS + the Q concept tokens of every image are carried; their
// residual rows are gathered into prune_into, which is c.H from there on.
template <class Launcher>
int ch_layer_forward(Launcher &run, ChChain &c, const LayerW &w, const ChLayerBufs &b, float *cattn, float *prune_into) {
    const int D = c.D, M = c.M;
    ChGemmCall g{3 * D, D, b.Xn1, b.qkv_folded ? w.qkv_wf : w.qkv_w, b.qkv_folded ? w.qkv_d : w.qkv_b, b.qkv_folded ? EPI_FOLD_BIAS : EPI_BIAS};
    g.cat = CH_CAT_GEMM_QKV; g.out = b.QKV; g.ldo = 3 * D;
    if (b.qkv_folded) { g.stats_in = b.st1; g.fold_c = w.qkv_c; g.eps = c.ln_eps; }
    if (int e = run.gemm(c.cur, g)) return e;
    if (int e = run.attention(b.QKV, b.AO, cattn, prune_into != nullptr)) return e;   // keys / values still cover every token
    if (prune_into) {
        if (int e = run.gather_head_rows(c.H, prune_into)) return e;
        c.cur = c.B * (1 + c.Q);
        c.H = prune_into;
    }
    // h = r + a + adapter_1(a): the residual add of `a` is the adapter's up-projection epilogue
    g = ChGemmCall{D, D, b.AO, w.out_w, w.out_b, EPI_BIAS_STATS};
    g.cat = CH_CAT_GEMM_OUT; g.out = b.A; g.ldo = D; g.stats_out = b.stA;
    if (int e = run.gemm(c.cur, g)) return e;
    if (int e = ch_adapter_forward(run, c, w.ad[0], b.A, b.stA, b.AD[0], b.ADpre[0], b.Xn2, b.st2)) return e;
    const int act1 = c.act == 0 ? EPI_FOLD_QUICKGELU : EPI_FOLD_GELU, act2 = c.act == 0 ? EPI_FOLD_ACT2_QUICK : EPI_FOLD_ACT2_GELU;
    g = ChGemmCall{M, D, b.Xn2, w.fc1_wf, w.fc1_d, b.F1pre ? act2 : act1};
    g.cat = CH_CAT_GEMM_FC1; g.stats_in = b.st2; g.fold_c = w.fc1_c; g.eps = c.ln_eps; g.out = b.F1pre ? b.F1pre : b.F1; g.ldo = M;
    if (b.F1pre) { g.hb_out = b.F1; g.ld_hb = M; }
    if (int e = run.gemm(c.cur, g)) return e;
    g = ChGemmCall{D, M, b.F1, w.fc2_w, w.fc2_b, EPI_BIAS_STATS};
    g.cat = CH_CAT_GEMM_FC2; g.out = b.A2; g.ldo = D; g.stats_out = b.stA2;
    if (int e = run.gemm(c.cur, g)) return e;
    return ch_adapter_forward(run, c, w.ad[1], b.A2, b.stA2, b.AD[1], b.ADpre[1], b.Xn_next, b.st_next);
}
