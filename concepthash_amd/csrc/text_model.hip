// ch_text: the CLIP TEXT tower on the GPU (C-ABI in include/concepthash_hip.h) -- what the reference's language-guided codebook
// (trainers/orthohash.py:94-145, codebook_method "L") runs once per training run: token + position embedding, L pre-LN layers
// with CAUSAL self-attention, final_layer_norm, and the EOS token's row as `pooler_output` (HF CLIPTextTransformer; there is no
// text projection on this path).  A text layer is the image tower's plain block (model.hip run_chain without adapters and
// without the LayerNorm fold), so the chain below is made of the same launchers: ch_layernorm_f32, ch_gemm_bf16 (whatever kernel
// the dispatcher picks for these shapes), the resident attention kernel's causal instance.  Precision policy as DESIGN.md
// section 3: bf16 GEMM operands, fp32 accumulation, fp32 residual stream, fp32 LayerNorm / softmax / pooling.
// There is no padding mask: the reference passes input_ids only, and causality alone keeps the padding behind EOS away from it.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/concepthash_hip.h"
#include "ch_common.h"
#include "kernels.h"
#include "weight_builder.h"

struct TextLayerW {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    const bf16_t *qkv_w, *out_w, *fc1_w, *fc2_w;   // [3D, D] (q | k | v), [D, D], [M, D], [D, M]
    const float *qkv_b, *out_b, *fc1_b, *fc2_b;
};

struct ch_text {
    ch_text_config cfg;
    ChDeviceOwner own;                                // every device block, the pinned `stage` and the `staged` event
    const float *tok = nullptr, *pos = nullptr;       // [vocab, D], [max_positions, D] fp32
    const float *fln_w = nullptr, *fln_b = nullptr;   // final_layer_norm
    std::vector<TextLayerW> layers;
    // workspace: rows padded to the GEMMs' block tile; padding rows are zero or stale finite values and never read back
    int64_t rows_alloc = 0;
    float *H = nullptr;
    bf16_t *Xn = nullptr, *QKV = nullptr, *AO = nullptr, *A = nullptr, *F1 = nullptr;
    int32_t *ids = nullptr, *eos = nullptr;           // device copies of the call's host arrays
    int32_t *stage = nullptr;                         // pinned host copy of both ([max_batch * max_positions] ids, then [max_batch] eos)
    hipEvent_t staged = nullptr;                      // recorded behind the copies out of `stage`: the next call waits for it before refilling
};

namespace {

constexpr int MAXP = 10;  // D <= 1280, D % 128 == 0 (the row kernels of rowops.hip)

// H[b*T + t] = token_embedding[ids[b, t]] + position_embedding[t]: one wave per row, 16-byte accesses.  ids were range-checked on the host.
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t *__restrict__ ids, int rows, int T, int D, const float *__restrict__ tok,
                                                         const float *__restrict__ pos, float *__restrict__ H) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = row % T;
    const float *te = tok + (size_t)ids[row] * D, *pe = pos + (size_t)t * D;
    float *dst = H + (size_t)row * D;
    for (int i = lane * 4; i < D; i += 256) {
        const f32x4 a = *(const f32x4 *)(te + i), b = *(const f32x4 *)(pe + i);
        *(f32x4 *)(dst + i) = a + b;
    }
}

// out[r] = LayerNorm_final(H[src(r)]) in fp32, one wave per output row, two-pass mean / variance like torch's layer_norm.
// eos != nullptr: r is a prompt and src = r*T + eos[r] (pooler_output); eos == nullptr: src = r (every row: the test output)
__global__ __launch_bounds__(256) void text_pool_kernel(const float *__restrict__ H, const int32_t *__restrict__ eos, int nrows, int T, int D,
                                                        const float *__restrict__ w, const float *__restrict__ b, float eps,
                                                        float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nrows) return;
    const size_t src = eos ? (size_t)r * T + eos[r] : (size_t)r;
    const float *x = H + src * D;
    const int npass = D >> 7;
    float2 v[MAXP];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXP; ++j)
        if (j < npass) {
            v[j] = *(const float2 *)(x + (j * 64 + lane) * 2);
            s += v[j].x + v[j].y;
        }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < MAXP; ++j)
        if (j < npass) {
            const float a = v[j].x - mean, c = v[j].y - mean;
            q += a * a + c * c;
        }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    float *dst = out + (size_t)r * D;
#pragma unroll
    for (int j = 0; j < MAXP; ++j)
        if (j < npass) {
            const int i = (j * 64 + lane) * 2;
            const float2 ww = *(const float2 *)(w + i), bb = *(const float2 *)(b + i);
            *(float2 *)(dst + i) = make_float2((v[j].x - mean) * rstd * ww.x + bb.x, (v[j].y - mean) * rstd * ww.y + bb.y);
        }
}

int validate(const ch_text_config *c) {
    CH_REQUIRE(c != nullptr, "null text config");
    CH_REQUIRE(c->dim > 0 && c->dim % 64 == 0, "text: dim must be a multiple of 64 (heads of 64)");
    CH_REQUIRE(c->dim % 128 == 0 && c->dim <= 1280, "text: dim must be a multiple of 128 and <= 1280 (LayerNorm rows, GEMM tiles)");
    CH_REQUIRE(c->heads > 0 && c->dim == c->heads * 64, "text: head_dim must be 64 (dim == heads * 64)");
    CH_REQUIRE(c->ffn > 0 && c->ffn % 128 == 0, "text: ffn must be a multiple of 128");
    CH_REQUIRE(c->layers >= 1, "text: layers must be >= 1");
    CH_REQUIRE(c->vocab >= 1, "text: vocab must be >= 1");
    CH_REQUIRE(c->max_positions >= 1 && c->max_positions <= CH_ATTN_RESIDENT_MAX_TOKENS,
               "text: max_positions must be in [1, 288] (the LDS-resident attention kernel; CLIP's 77 run its 96-key instance, and past 128 "
               "positions the causal instances hold one wave per SIMD fewer than the plain ones or, past 256, spill like them: DESIGN.md 3.12)");
    CH_REQUIRE(c->act == 0 || c->act == 1, "text: act must be 0 (quick_gelu) or 1 (gelu)");
    CH_REQUIRE(c->max_batch >= 1, "text: max_batch must be >= 1");
    return 0;
}

int build_text(ch_text *m, const ch_tensor *tensors, int ntensors) {
    const ch_text_config &c = m->cfg;
    ChWeightBuilder B(m->own);
    for (int i = 0; i < ntensors; ++i) {
        CH_REQUIRE(tensors[i].name && tensors[i].data, "tensor entry with null name/data");
        B.tab[tensors[i].name] = &tensors[i];
    }
    const int D = c.dim, M = c.ffn;
    const std::string TM = "text_model.";
    m->tok = B.f32(TM + "embeddings.token_embedding.weight", (int64_t)c.vocab * D);
    m->pos = B.f32(TM + "embeddings.position_embedding.weight", (int64_t)c.max_positions * D);
    m->fln_w = B.f32(TM + "final_layer_norm.weight", D);
    m->fln_b = B.f32(TM + "final_layer_norm.bias", D);
    m->layers.resize(c.layers);
    for (int i = 0; i < c.layers && B.ok; ++i) {
        const std::string pre = TM + "encoder.layers." + std::to_string(i) + ".";
        TextLayerW &w = m->layers[i];
        w.ln1_w = B.f32(pre + "layer_norm1.weight", D);
        w.ln1_b = B.f32(pre + "layer_norm1.bias", D);
        w.ln2_w = B.f32(pre + "layer_norm2.weight", D);
        w.ln2_b = B.f32(pre + "layer_norm2.bias", D);
        bf16_t *qkvw = (bf16_t *)B.alloc(sizeof(bf16_t) * 3 * D * D);
        float *qkvb = (float *)B.alloc(sizeof(float) * 3 * D);
        if (!B.ok) break;
        const char *names[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3 && B.ok; ++j) {
            B.bf16(pre + "self_attn." + names[j] + ".weight", D, D, D, qkvw + (size_t)j * D * D);
            B.f32(pre + "self_attn." + names[j] + ".bias", D, qkvb + (size_t)j * D);
        }
        w.qkv_w = qkvw;
        w.qkv_b = qkvb;
        w.out_w = B.bf16(pre + "self_attn.out_proj.weight", D, D, D);
        w.out_b = B.f32(pre + "self_attn.out_proj.bias", D);
        w.fc1_w = B.bf16(pre + "mlp.fc1.weight", M, D, D);
        w.fc1_b = B.f32(pre + "mlp.fc1.bias", M);
        w.fc2_w = B.bf16(pre + "mlp.fc2.weight", D, M, M);
        w.fc2_b = B.f32(pre + "mlp.fc2.bias", D);
    }
    if (!B.ok) return 4;
    for (const auto &kv : B.tab)   // position_ids is an index buffer older checkpoints carry, not a weight
        if (!B.used.count(kv.first) && kv.first != TM + "embeddings.position_ids") {
            ch_set_error("unknown tensor '" + kv.first + "'");
            return 4;
        }
    const int64_t rows = round_up64((int64_t)c.max_batch * c.max_positions, 256) + 256;   // +256: a last tile's over-read
    m->rows_alloc = rows;
    m->H = (float *)B.alloc(sizeof(float) * rows * D, true);
    m->Xn = (bf16_t *)B.alloc(sizeof(bf16_t) * rows * D, true);
    m->QKV = (bf16_t *)B.alloc(sizeof(bf16_t) * rows * 3 * D, true);
    m->AO = (bf16_t *)B.alloc(sizeof(bf16_t) * rows * D, true);
    m->A = (bf16_t *)B.alloc(sizeof(bf16_t) * rows * D, true);
    m->F1 = (bf16_t *)B.alloc(sizeof(bf16_t) * rows * M, true);
    m->ids = (int32_t *)B.alloc(sizeof(int32_t) * (size_t)c.max_batch * c.max_positions, true);
    m->eos = (int32_t *)B.alloc(sizeof(int32_t) * (size_t)c.max_batch, true);
    if (!B.ok) return 4;
    m->stage = (int32_t *)m->own.host_alloc(sizeof(int32_t) * ((size_t)c.max_batch * c.max_positions + c.max_batch));
    m->staged = m->own.event(hipEventDisableTiming);
    if (!m->stage || !m->staged) return 1;
    CH_CHECK_HIP(hipDeviceSynchronize());
    return 0;
}

int run_text(ch_text *m, int B, int T, float *out_pooled, float *out_hidden, hipStream_t s) {
    const ch_text_config &c = m->cfg;
    const int D = c.dim, M = c.ffn, rows = B * T;
    const int act_epi = c.act == 0 ? EPI_BIAS_QUICKGELU : EPI_BIAS_GELU;
    if (int e = ch_text_embed(m->ids, rows, T, D, m->tok, m->pos, m->H, s)) return e;
    auto gemm = [&](const bf16_t *X, const bf16_t *W, int N, int K, const float *bias, int epi, bf16_t *out, int ldo) {
        GemmParams p{};
        p.X = X; p.W = W; p.M = rows; p.N = N; p.K = K; p.X_rows_alloc = m->rows_alloc; p.bias = bias;
        p.out_bf16 = out; p.ldo = ldo; p.resid = m->H; p.ldr = D;
        return ch_gemm_bf16(p, epi, s);
    };
    for (const TextLayerW &w : m->layers) {
        if (int e = ch_layernorm_f32(m->H, rows, D, w.ln1_w, w.ln1_b, c.ln_eps, m->Xn, s)) return e;
        if (int e = gemm(m->Xn, w.qkv_w, 3 * D, D, w.qkv_b, EPI_BIAS, m->QKV, 3 * D)) return e;
        if (int e = ch_attention_causal(m->QKV, B, T, c.heads, m->AO, s)) return e;
        if (int e = gemm(m->AO, w.out_w, D, D, w.out_b, EPI_BIAS_RESID, m->A, D)) return e;
        if (int e = ch_layernorm_f32(m->H, rows, D, w.ln2_w, w.ln2_b, c.ln_eps, m->Xn, s)) return e;
        if (int e = gemm(m->Xn, w.fc1_w, M, D, w.fc1_b, act_epi, m->F1, M)) return e;
        if (int e = gemm(m->F1, w.fc2_w, D, M, w.fc2_b, EPI_BIAS_RESID, m->A, D)) return e;
    }
    if (int e = ch_text_pool(m->H, m->eos, B, T, D, m->fln_w, m->fln_b, c.ln_eps, out_pooled, s)) return e;
    if (out_hidden)
        if (int e = ch_text_pool(m->H, nullptr, rows, T, D, m->fln_w, m->fln_b, c.ln_eps, out_hidden, s)) return e;
    return 0;
}

}  // namespace

// the launchers of the two kernels (kernels.h): what run_text calls, and what the taps of debug_taps.hip launch on caller buffers
int ch_text_embed(const int32_t *ids, int rows, int T, int D, const float *tok, const float *pos, float *H, hipStream_t s) {
    CH_REQUIRE(D > 0 && D % 128 == 0 && D <= 128 * MAXP, "text_embed: D must be a multiple of 128 and <= 1280");
    CH_REQUIRE(rows >= 1 && T >= 1, "text_embed: rows and T must be >= 1");
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)ceil_div64(rows, 4)), dim3(256), 0, s, ids, rows, T, D, tok, pos, H);
    CH_LAUNCH_CHECK();
    return 0;
}

int ch_text_pool(const float *H, const int32_t *eos, int nrows, int T, int D, const float *w, const float *b, float eps, float *out,
                 hipStream_t s) {
    CH_REQUIRE(D > 0 && D % 128 == 0 && D <= 128 * MAXP, "text_pool: D must be a multiple of 128 and <= 1280");
    CH_REQUIRE(nrows >= 1 && T >= 1, "text_pool: nrows and T must be >= 1");
    hipLaunchKernelGGL(text_pool_kernel, dim3((unsigned)ceil_div64(nrows, 4)), dim3(256), 0, s, H, eos, nrows, T, D, w, b, eps, out);
    CH_LAUNCH_CHECK();
    return 0;
}

extern "C" int ch_text_create(const ch_text_config *cfg, const ch_tensor *tensors, int32_t ntensors, ch_text **out) {
    CH_REQUIRE(out != nullptr, "null out pointer");
    *out = nullptr;
    if (int e = validate(cfg)) return e;
    CH_REQUIRE(tensors != nullptr && ntensors > 0, "no tensors");
    ch_text *m = new ch_text();
    m->cfg = *cfg;
    if (m->cfg.ln_eps <= 0.f) m->cfg.ln_eps = 1e-5f;
    if (int e = build_text(m, tensors, ntensors)) {
        ch_text_destroy(m);
        return e;
    }
    *out = m;
    return 0;
}

extern "C" void ch_text_destroy(ch_text *m) {
    delete m;
}

extern "C" size_t ch_text_device_bytes(const ch_text *m) { return m ? m->own.bytes() : 0; }

extern "C" int ch_text_encode(ch_text *m, const int32_t *ids, const int32_t *eos_pos, int32_t B, int32_t T, float *out_pooled,
                              float *out_hidden, void *stream) {
    CH_REQUIRE(m != nullptr, "text_encode: null handle");
    CH_REQUIRE(ids && eos_pos && out_pooled, "text_encode: null pointer");
    CH_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "text_encode: B must be in [1, max_batch]");
    CH_REQUIRE(T >= 1 && T <= m->cfg.max_positions, "text_encode: T must be in [1, max_positions]");
    for (int64_t i = 0; i < (int64_t)B * T; ++i)
        CH_REQUIRE(ids[i] >= 0 && ids[i] < m->cfg.vocab, "text_encode: token id " + std::to_string(ids[i]) + " at position " + std::to_string(i) +
                                                             " is outside [0, vocab)");
    for (int b = 0; b < B; ++b)
        CH_REQUIRE(eos_pos[b] >= 0 && eos_pos[b] < T, "text_encode: eos_pos " + std::to_string(eos_pos[b]) + " of prompt " + std::to_string(b) +
                                                          " is outside [0, T)");
    hipStream_t s = (hipStream_t)stream;
    // the arrays are copied into the handle's pinned buffer here, so the caller may reuse them as soon as the call returns; the
    // buffer is refilled only after the previous call's copies out of it have executed
    CH_CHECK_HIP(hipEventSynchronize(m->staged));
    int32_t *eos_stage = m->stage + (size_t)m->cfg.max_batch * m->cfg.max_positions;
    std::copy(ids, ids + (size_t)B * T, m->stage);
    std::copy(eos_pos, eos_pos + B, eos_stage);
    CH_CHECK_HIP(hipMemcpyAsync(m->ids, m->stage, sizeof(int32_t) * (size_t)B * T, hipMemcpyHostToDevice, s));
    CH_CHECK_HIP(hipMemcpyAsync(m->eos, eos_stage, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, s));
    CH_CHECK_HIP(hipEventRecord(m->staged, s));
    return run_text(m, B, T, out_pooled, out_hidden, s);
}
