// GEMM epilogue numbers and the per-layer weight structs: plain C++ (no HIP), so that layer_forward.h compiles in a CPU test.
#pragma once
#include <stdint.h>

typedef uint16_t bf16_t;  // raw bf16 bits

// ---- gemm_bf16.hip (the numbers are part of the debug taps' interface: they do not change)
enum GemmEpilogue {
    EPI_BIAS = 0,           // out_bf16 = acc + bias
    EPI_BIAS_QUICKGELU = 1, // out_bf16 = quick_gelu(acc + bias)
    EPI_BIAS_GELU = 2,      // out_bf16 = gelu_erf(acc + bias)
    EPI_BIAS_RESID = 3,     // v = acc + bias; resid += v; out_bf16 = v
    EPI_SCALE_RESID = 4,    // resid += [addend] + *scale_ptr * (acc + bias)
    EPI_PATCH = 5,          // resid[token row of patch m] = acc + pos[1 + patch]
    // ---- LayerNorm folded into the CONSUMER GEMM: the producer of a LayerNorm input emits per-row
    // partial (sum, sum of squares) over each 64-column slice of its bf16-rounded output; the consumer multiplies the RAW
    // rows by W' = bf16(W * gamma) and normalises in its epilogue:  y = rstd_m * (acc - mean_m * c_n) + d_n,
    // c_n = sum_k W'[n][k], d_n = bias_n + sum_k W[n][k] * beta_k.
    EPI_BIAS_STATS = 6,         // EPI_BIAS + row statistics of out_bf16 -> stats_out
    EPI_SCALE_RESID_STATS = 7,  // EPI_SCALE_RESID + hb_out = bf16(resid) + row statistics of hb_out -> stats_out
    EPI_FOLD_BIAS = 8,          // out_bf16 = LN-folded linear (bias = d, fold_c = c, stats_in)
    EPI_FOLD_QUICKGELU = 9,     // ... then quick_gelu
    EPI_FOLD_GELU = 10,         // ... then gelu_erf
    // ---- training step (train.hip): activations applied / differentiated on a bf16 PRE-activation tensor in the epilogue
    EPI_BIAS_DACT_QUICK = 11,   // out_bf16 = bf16(acc + bias) * quick_gelu'(aux)                     (fc2 input-gradient GEMM)
    EPI_BIAS_DACT_GELU = 12,    // out_bf16 = *scale_ptr * bf16(acc + bias) * gelu_erf'(aux)          (adapter up-projection dgrad)
    EPI_FOLD_ACT2_QUICK = 13,   // out_bf16 = pre = LN-folded linear; hb_out = quick_gelu(pre)        (fc1 forward, pre kept for backward)
    EPI_FOLD_ACT2_GELU = 14,    // ... hb_out = gelu_erf(pre)                                          (adapter down-projection forward)
    EPI_COUNT = 15,
};

struct AdapterW {
    const float *ln_w = nullptr, *ln_b = nullptr, *down_b = nullptr, *up_b = nullptr, *scale = nullptr;
    const bf16_t *down_w = nullptr, *up_w = nullptr;
    // adapter LayerNorm folded into the down projection (LN-fold chain and adapter_fused.hip)
    const bf16_t *down_wf = nullptr;
    const float *fold_c = nullptr, *fold_d = nullptr;
};
struct LayerW {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *qkv_b, *out_b, *fc1_b, *fc2_b;
    const bf16_t *qkv_w, *out_w, *fc1_w, *fc2_w;
    // layer_norm1 / layer_norm2 folded into qkv / fc1: W' = bf16(W * gamma), c = row sums of W', d = bias + W beta
    const bf16_t *qkv_wf = nullptr, *fc1_wf = nullptr;
    const float *qkv_c = nullptr, *qkv_d = nullptr, *fc1_c = nullptr, *fc1_d = nullptr;
    AdapterW ad[2];
};
