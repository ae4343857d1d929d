// CPU test of csrc/layer_forward.h (tests/test_layer_forward_cpu.py builds this with g++ -fsanitize=address,undefined and runs it):
// the header the library compiles, instantiated over a launcher that records every call.  The expected launch sequences below were
// written out from the two hand-written chains this header replaced (run_chain of model.hip for the encode cases, forward_chain of
// train.hip for the training ones), call by call -- not from the header.  Usage: layer_forward_test CASE; exit status 0 and a line
// "ok CASE" on success.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "layer_forward.h"

enum Kind { GEMM, ATTENTION, GATHER };
struct Rec {
    int kind = GEMM, rows = 0, cat = 0, epi = 0, N = 0, K = 0, n_true = 0, k_true = 0;
    const void *X = nullptr, *W = nullptr, *bias = nullptr, *out = nullptr;
    int ldo = 0;
    const void *resid = nullptr, *scale = nullptr, *addend = nullptr, *stats_in = nullptr, *fold_c = nullptr;
    float eps = 0.f;
    const void *stats_out = nullptr, *hb_out = nullptr;
    int ld_hb = 0;
    const void *aux = nullptr, *cattn = nullptr, *gather_to = nullptr;   // attention: X = qkv; gather: resid = H
    bool compact = false;
    // named setters, so that an expected record reads like the call it stands for
    Rec &fold(const void *st, const void *c, float e) { stats_in = st; fold_c = c; eps = e; return *this; }
    Rec &stats(const void *st) { stats_out = st; return *this; }
    Rec &hb(const void *p, int ld) { hb_out = p; ld_hb = ld; return *this; }
    Rec &res(const void *r, const void *s, const void *a) { resid = r; scale = s; addend = a; return *this; }
    bool operator==(const Rec &o) const {
        return kind == o.kind && rows == o.rows && cat == o.cat && epi == o.epi && N == o.N && K == o.K && n_true == o.n_true && k_true == o.k_true &&
               X == o.X && W == o.W && bias == o.bias && out == o.out && ldo == o.ldo && resid == o.resid && scale == o.scale && addend == o.addend &&
               stats_in == o.stats_in && fold_c == o.fold_c && eps == o.eps && stats_out == o.stats_out && hb_out == o.hb_out && ld_hb == o.ld_hb &&
               aux == o.aux && cattn == o.cattn && gather_to == o.gather_to && compact == o.compact;
    }
};
static Rec G(int rows, int cat, int epi, int N, int K, int n_true, int k_true, const void *X, const void *W, const void *bias, const void *out, int ldo) {
    Rec r;
    r.rows = rows; r.cat = cat; r.epi = epi; r.N = N; r.K = K; r.n_true = n_true; r.k_true = k_true; r.X = X; r.W = W; r.bias = bias; r.out = out; r.ldo = ldo;
    return r;
}
static Rec A(const void *qkv, const void *out, const void *cattn, bool compact) {
    Rec r;
    r.kind = ATTENTION; r.X = qkv; r.out = out; r.cattn = cattn; r.compact = compact;
    return r;
}
static Rec Gather(const void *H, const void *Hc) {
    Rec r;
    r.kind = GATHER; r.resid = H; r.gather_to = Hc;
    return r;
}

struct Recorder {
    std::vector<Rec> log;
    int gemm(int rows, const ChGemmCall &g) {
        Rec r = G(rows, g.cat, g.epi, g.N, g.K, g.n_true ? g.n_true : g.N, g.k_true ? g.k_true : g.K, g.X, g.W, g.bias, g.out, g.ldo);
        r.res(g.resid, g.scale, g.addend).fold(g.stats_in, g.fold_c, g.eps).stats(g.stats_out).hb(g.hb_out, g.ld_hb);
        r.aux = g.aux;
        log.push_back(r);
        return 0;
    }
    int attention(const bf16_t *qkv, bf16_t *out, float *cattn, bool compact) {
        log.push_back(A(qkv, out, cattn, compact));
        return 0;
    }
    int gather_head_rows(const float *H, float *Hc) {
        log.push_back(Gather(H, Hc));
        return 0;
    }
};

// ---- fake operands: one object per buffer, so that every pointer is distinct and names itself
static struct {
    bf16_t qkv_w, qkv_wf, out_w, fc1_w, fc1_wf, fc2_w, down_wf[2], up_w[2];
    float qkv_b, qkv_c, qkv_d, out_b, fc1_b, fc1_c, fc1_d, fc2_b, fold_c[2], fold_d[2], up_b[2], scale[2];
} W;
static struct {   // ch_encode: one set of buffers for every layer
    bf16_t Xn, QKV, AO, A, AD, F1;
    float statsH, statsA, H, Hc, tap;
} E;
static struct {   // training: buffers of layer l, the next layer's LayerNorm input, the dummies behind the last layer
    bf16_t Xn1, QKV, AO, A, P1, G1, Xn2, F1pre, F1act, A2, P2, G2, Xn1_next, XnDummy;
    float st1, stA, st2, stA2, st1_next, stDummy, H, Hc, tap;
} T;

constexpr int D = 128, M = 512, BPAD = 128, AD_DIM = 64, Q = 2, NTOK = 5, B = 2, ROWS = B * NTOK, PRUNED = B * (1 + Q);
constexpr float LN_EPS = 1e-6f, AD_EPS = 1e-5f;

static LayerW weights() {
    LayerW w{};
    w.qkv_w = &W.qkv_w; w.qkv_b = &W.qkv_b; w.qkv_wf = &W.qkv_wf; w.qkv_c = &W.qkv_c; w.qkv_d = &W.qkv_d;
    w.out_w = &W.out_w; w.out_b = &W.out_b; w.fc1_w = &W.fc1_w; w.fc1_b = &W.fc1_b; w.fc1_wf = &W.fc1_wf; w.fc1_c = &W.fc1_c; w.fc1_d = &W.fc1_d;
    w.fc2_w = &W.fc2_w; w.fc2_b = &W.fc2_b;
    for (int a = 0; a < 2; ++a) {
        w.ad[a].down_wf = &W.down_wf[a]; w.ad[a].fold_c = &W.fold_c[a]; w.ad[a].fold_d = &W.fold_d[a];
        w.ad[a].up_w = &W.up_w[a]; w.ad[a].up_b = &W.up_b[a]; w.ad[a].scale = &W.scale[a];
    }
    return w;
}
// the buffers as run_chain hands them in: Xn / statsH and A / statsA serve every role; no pre-activations
static ChLayerBufs encode_bufs(bool qkv_folded, bool last) {
    ChLayerBufs b{};
    b.Xn1 = b.Xn2 = &E.Xn; b.st1 = b.st2 = &E.statsH; b.qkv_folded = qkv_folded; b.QKV = &E.QKV; b.AO = &E.AO;
    b.A = b.A2 = &E.A; b.stA = b.stA2 = &E.statsA; b.AD[0] = b.AD[1] = &E.AD; b.F1 = &E.F1;
    if (!last) { b.Xn_next = &E.Xn; b.st_next = &E.statsH; }
    return b;
}
// ... and as forward_chain does: everything per layer, both pre-activation sets, the dummies behind the last layer
static ChLayerBufs train_bufs(bool last) {
    ChLayerBufs b{};
    b.Xn1 = &T.Xn1; b.st1 = &T.st1; b.qkv_folded = true; b.QKV = &T.QKV; b.AO = &T.AO; b.A = &T.A; b.stA = &T.stA; b.A2 = &T.A2; b.stA2 = &T.stA2;
    b.AD[0] = &T.G1; b.ADpre[0] = &T.P1; b.AD[1] = &T.G2; b.ADpre[1] = &T.P2; b.Xn2 = &T.Xn2; b.st2 = &T.st2; b.F1 = &T.F1act; b.F1pre = &T.F1pre;
    b.Xn_next = last ? &T.XnDummy : &T.Xn1_next; b.st_next = last ? &T.stDummy : &T.st1_next;
    return b;
}

// ---- expected sequences
// run_chain, LN-fold chain.  qkv: layer 0 is the plain GEMM on rows ch_assemble_preln normalised, later layers the folded one on
// (Xn, statsH).  `rows` / `H` after the attention: all token rows and m->H, or the compact head rows and Hc when the layer prunes.
static std::vector<Rec> expect_encode(bool qkv_folded, bool last, bool prunes, int fc1_epi) {
    const int r = prunes ? PRUNED : ROWS;
    const float *H = prunes ? &E.Hc : &E.H;
    std::vector<Rec> v;
    if (qkv_folded) v.push_back(G(ROWS, CH_CAT_GEMM_QKV, EPI_FOLD_BIAS, 3 * D, D, 3 * D, D, &E.Xn, &W.qkv_wf, &W.qkv_d, &E.QKV, 3 * D).fold(&E.statsH, &W.qkv_c, LN_EPS));
    else v.push_back(G(ROWS, CH_CAT_GEMM_QKV, EPI_BIAS, 3 * D, D, 3 * D, D, &E.Xn, &W.qkv_w, &W.qkv_b, &E.QKV, 3 * D));
    v.push_back(A(&E.QKV, &E.AO, &E.tap, prunes));
    if (prunes) v.push_back(Gather(&E.H, &E.Hc));
    v.push_back(G(r, CH_CAT_GEMM_OUT, EPI_BIAS_STATS, D, D, D, D, &E.AO, &W.out_w, &W.out_b, &E.A, D).stats(&E.statsA));
    v.push_back(G(r, CH_CAT_GEMM_DOWN, EPI_FOLD_GELU, BPAD, D, AD_DIM, D, &E.A, &W.down_wf[0], &W.fold_d[0], &E.AD, BPAD).fold(&E.statsA, &W.fold_c[0], AD_EPS));
    v.push_back(G(r, CH_CAT_GEMM_UP, EPI_SCALE_RESID_STATS, D, BPAD, D, AD_DIM, &E.AD, &W.up_w[0], &W.up_b[0], nullptr, 0).res(H, &W.scale[0], &E.A).stats(&E.statsH).hb(&E.Xn, 0));
    v.push_back(G(r, CH_CAT_GEMM_FC1, fc1_epi, M, D, M, D, &E.Xn, &W.fc1_wf, &W.fc1_d, &E.F1, M).fold(&E.statsH, &W.fc1_c, LN_EPS));
    v.push_back(G(r, CH_CAT_GEMM_FC2, EPI_BIAS_STATS, D, M, D, M, &E.F1, &W.fc2_w, &W.fc2_b, &E.A, D).stats(&E.statsA));
    v.push_back(G(r, CH_CAT_GEMM_DOWN, EPI_FOLD_GELU, BPAD, D, AD_DIM, D, &E.A, &W.down_wf[1], &W.fold_d[1], &E.AD, BPAD).fold(&E.statsA, &W.fold_c[1], AD_EPS));
    if (last) v.push_back(G(r, CH_CAT_GEMM_UP, EPI_SCALE_RESID, D, BPAD, D, AD_DIM, &E.AD, &W.up_w[1], &W.up_b[1], nullptr, 0).res(H, &W.scale[1], &E.A));
    else v.push_back(G(r, CH_CAT_GEMM_UP, EPI_SCALE_RESID_STATS, D, BPAD, D, AD_DIM, &E.AD, &W.up_w[1], &W.up_b[1], nullptr, 0).res(H, &W.scale[1], &E.A).stats(&E.statsH).hb(&E.Xn, 0));
    return v;
}
// forward_chain: qkv always folded; two-output epilogues (pre-activation in `out`, activation in hb_out with its own leading
// dimension); the second up-projection always writes statistics -- into the next layer's (Xn1, st1) or the dummies
static std::vector<Rec> expect_train(bool last, bool prunes, int fc1_epi) {
    const int r = prunes ? PRUNED : ROWS;
    const float *H = prunes ? &T.Hc : &T.H;
    std::vector<Rec> v;
    v.push_back(G(ROWS, CH_CAT_GEMM_QKV, EPI_FOLD_BIAS, 3 * D, D, 3 * D, D, &T.Xn1, &W.qkv_wf, &W.qkv_d, &T.QKV, 3 * D).fold(&T.st1, &W.qkv_c, LN_EPS));
    v.push_back(A(&T.QKV, &T.AO, &T.tap, prunes));
    if (prunes) v.push_back(Gather(&T.H, &T.Hc));
    v.push_back(G(r, CH_CAT_GEMM_OUT, EPI_BIAS_STATS, D, D, D, D, &T.AO, &W.out_w, &W.out_b, &T.A, D).stats(&T.stA));
    v.push_back(G(r, CH_CAT_GEMM_DOWN, EPI_FOLD_ACT2_GELU, BPAD, D, AD_DIM, D, &T.A, &W.down_wf[0], &W.fold_d[0], &T.P1, BPAD).fold(&T.stA, &W.fold_c[0], AD_EPS).hb(&T.G1, BPAD));
    v.push_back(G(r, CH_CAT_GEMM_UP, EPI_SCALE_RESID_STATS, D, BPAD, D, AD_DIM, &T.G1, &W.up_w[0], &W.up_b[0], nullptr, 0).res(H, &W.scale[0], &T.A).stats(&T.st2).hb(&T.Xn2, 0));
    v.push_back(G(r, CH_CAT_GEMM_FC1, fc1_epi, M, D, M, D, &T.Xn2, &W.fc1_wf, &W.fc1_d, &T.F1pre, M).fold(&T.st2, &W.fc1_c, LN_EPS).hb(&T.F1act, M));
    v.push_back(G(r, CH_CAT_GEMM_FC2, EPI_BIAS_STATS, D, M, D, M, &T.F1act, &W.fc2_w, &W.fc2_b, &T.A2, D).stats(&T.stA2));
    v.push_back(G(r, CH_CAT_GEMM_DOWN, EPI_FOLD_ACT2_GELU, BPAD, D, AD_DIM, D, &T.A2, &W.down_wf[1], &W.fold_d[1], &T.P2, BPAD).fold(&T.stA2, &W.fold_c[1], AD_EPS).hb(&T.G2, BPAD));
    v.push_back(G(r, CH_CAT_GEMM_UP, EPI_SCALE_RESID_STATS, D, BPAD, D, AD_DIM, &T.G2, &W.up_w[1], &W.up_b[1], nullptr, 0).res(H, &W.scale[1], &T.A2)
                    .stats(last ? &T.stDummy : &T.st1_next).hb(last ? &T.XnDummy : &T.Xn1_next, 0));
    return v;
}

static int check(const std::vector<Rec> &got, const std::vector<Rec> &want, const ChChain &c, int want_cur, const float *want_H) {
    if (got.size() != want.size()) return fprintf(stderr, "%zu calls recorded, %zu expected\n", got.size(), want.size()), 1;
    for (size_t i = 0; i < got.size(); ++i)
        if (!(got[i] == want[i]))
            return fprintf(stderr, "call %zu differs: kind %d/%d rows %d/%d cat %d/%d epi %d/%d N %d/%d K %d/%d (recorded/expected)\n", i, got[i].kind,
                           want[i].kind, got[i].rows, want[i].rows, got[i].cat, want[i].cat, got[i].epi, want[i].epi, got[i].N, want[i].N, got[i].K, want[i].K), 1;
    if (c.cur != want_cur || c.H != want_H) return fprintf(stderr, "chain state after the layer: cur %d (expected %d), H %s\n", c.cur, want_cur, c.H == want_H ? "ok" : "wrong"), 1;
    return 0;
}

int main(int argc, char **argv) {
    const std::string name = argc > 1 ? argv[1] : "";
    const LayerW w = weights();
    Recorder run;
    int bad = 1;
    auto chain = [&](int act, float *H) { return ChChain{B, NTOK, Q, D, M, BPAD, AD_DIM, act, LN_EPS, ROWS, H}; };
    if (name == "encode_layer0" || name == "encode_middle" || name == "encode_last_pruned" || name == "encode_last" || name == "encode_gelu") {
        const bool folded = name != "encode_layer0", last = name == "encode_last_pruned" || name == "encode_last", prunes = name == "encode_last_pruned";
        ChChain c = chain(name == "encode_gelu" ? 1 : 0, &E.H);
        if (ch_layer_forward(run, c, w, encode_bufs(folded, last), &E.tap, prunes ? &E.Hc : nullptr)) return 1;
        bad = check(run.log, expect_encode(folded, last, prunes, name == "encode_gelu" ? EPI_FOLD_GELU : EPI_FOLD_QUICKGELU), c, prunes ? PRUNED : ROWS,
                    prunes ? &E.Hc : &E.H);
    } else if (name == "train_middle" || name == "train_last_pruned" || name == "train_gelu") {
        const bool last = name == "train_last_pruned";
        ChChain c = chain(name == "train_gelu" ? 1 : 0, &T.H);
        if (ch_layer_forward(run, c, w, train_bufs(last), &T.tap, last ? &T.Hc : nullptr)) return 1;
        bad = check(run.log, expect_train(last, last, name == "train_gelu" ? EPI_FOLD_ACT2_GELU : EPI_FOLD_ACT2_QUICK), c, last ? PRUNED : ROWS, last ? &T.Hc : &T.H);
    } else {
        fprintf(stderr, "unknown case '%s'\n", name.c_str());
    }
    if (bad) return 1;
    printf("ok %s\n", name.c_str());
    return 0;
}
