// TrivialAugmentWide training chain on the GPU (reference configs/transforms/trivialaugment.yaml):
//   Resize(resize, BILINEAR, shorter side) -> RandomHorizontalFlip -> TrivialAugmentWide(bicubic, fill None) -> CenterCrop(crop)
//   -> ToTensor -> normalize.
// The random draws (flip, op, signed magnitude) are the loader's, made with the CPU chain's random calls; the host turns them into
// per-image parameters exactly as torchvision / Pillow do (utils.transforms.ta_op_params) and stages them in ch_augment_desc.  Here:
//   1. ta_resize_h / ta_resize_v: Pillow's ImagingResample with the triangle filter (support 1): double-precision coefficients
//      normalised and quantised to 22 fractional bits, two passes with an 8-bit intermediate -- the bicubic restatement of
//      preprocess.hip with the other filter.  The FULL resized image is written (the ops read outside the crop: statistics, the
//      geometric ops' sources), mirrored when the flip was drawn;
//   2. ta_lut: one workgroup per image whose op is a per-channel table (Identity, rotate's copy path, Brightness, Contrast,
//      Posterize, Solarize, AutoContrast, Equalize): the histograms the op needs (L for Contrast's mean, per channel for
//      AutoContrast / Equalize) over the whole resized image, then the table with Pillow's integer / double / float arithmetic;
//   3. ta_output: only the crop x crop window -- the table, Color (L by Pillow's fixed-point weights, then blend), Sharpness (3x3
//      SMOOTH with its border rule, then blend), the bicubic affine sampler (ShearX/Y, TranslateX/Y, Rotate) in double precision,
//      or rotate's transpose fast paths -- then ToTensor + normalise as ch_preprocess does.
// Floating-point contraction is off: every double / float operation is the one Pillow's C code performs (pinned in numpy against
// Pillow by tests/test_trivialaugment_cpu.py).
#pragma clang fp contract(off)
#include "../../include/concepthash_hip.h"
#include "ch_common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int KMAX = 64;      // taps per output index: 2 * ceil(scale) + 1 <= 64 <=> down-scaling up to 31x
constexpr int HROWS = 16;     // source rows per workgroup of the horizontal pass
constexpr int LUT_BYTES = 3 * 256;

enum : int { OP_IDENTITY = 0, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST,
             OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE };
enum : int { ROT_AFFINE = 0, ROT_COPY = 1, ROT_90 = 2, ROT_270 = 3, ROT_180 = 4 };

__device__ __forceinline__ double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc (triangle filter) for ONE output index xx of a (0, in_size) -> out_size resize.
__device__ __forceinline__ int2 bilinear_coeffs(int in_size, int out_size, int xx, int *kk, int kstride) {
    const double scale = (double)((float)in_size - 0.0f) / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > KMAX) xmax = KMAX;  // unreachable: the host routes images that need more taps through Pillow
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bilinear_filter((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double w = bilinear_filter((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        kk[x * kstride] = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
    }
    return make_int2(xmin, xmax);
}

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Image.blend(im1, im2, alpha) per byte (ImagingBlend: alpha is a C float; 0 <= alpha <= 1 interpolates, else extrapolates and clips)
__device__ __forceinline__ int blend8(int in1, int in2, float alpha) {
    const float t = (float)in1 + alpha * (float)(in2 - in1);
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 255;
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (int)t;
}

__device__ __forceinline__ int rgb_to_l(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ bool uses_lut(int op, int iparam) {
    return op == OP_IDENTITY || (op == OP_ROTATE && iparam == ROT_COPY) || op == OP_BRIGHTNESS || op == OP_CONTRAST || op == OP_POSTERIZE ||
           op == OP_SOLARIZE || op == OP_AUTOCONTRAST || op == OP_EQUALIZE;
}

// horizontal pass: tmp[r][x][c] for the source rows r in [row0, row0 + nrows) and every column x of the resized width
__global__ __launch_bounds__(256) void ta_resize_h_kernel(const uint8_t *__restrict__ pixels, const ch_augment_desc *__restrict__ desc,
                                                          uint8_t *__restrict__ ws) {
    __shared__ int kk[KMAX * 256];  // [tap][thread]: each lane reads only its own column (no barrier)
    const ch_augment_desc &d = desc[blockIdx.x];
    const int nrows = d.nrows, w = d.w, nw = d.nw, row0 = d.row0;
    const int r_begin = blockIdx.y * HROWS;
    if (r_begin >= nrows) return;   // block-uniform (nrows = 0: host route)
    const int r_end = min(r_begin + HROWS, nrows);
    const uint8_t *src = pixels + d.src_offset;
    uint8_t *dst = ws + d.tmp_offset;
    for (int x = threadIdx.x; x < nw; x += 256) {
        const int2 b = bilinear_coeffs(w, nw, x, kk + threadIdx.x, 256);
        for (int r = r_begin; r < r_end; ++r) {
            const uint8_t *row = src + ((size_t)(row0 + r) * w + b.x) * 3;
            int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
            for (int t = 0; t < b.y; ++t) {
                const int k = kk[t * 256 + threadIdx.x];
                s0 += (int)row[t * 3 + 0] * k;
                s1 += (int)row[t * 3 + 1] * k;
                s2 += (int)row[t * 3 + 2] * k;
            }
            uint8_t *o = dst + ((size_t)r * nw + x) * 3;
            o[0] = (uint8_t)clip8(s0);
            o[1] = (uint8_t)clip8(s1);
            o[2] = (uint8_t)clip8(s2);
        }
    }
}

// vertical pass: img[y][x'][c] of the whole resized image, x' = nw - 1 - x when the flip was drawn
__global__ __launch_bounds__(256) void ta_resize_v_kernel(const ch_augment_desc *__restrict__ desc, uint8_t *__restrict__ ws) {
    __shared__ int kk[KMAX];
    __shared__ int2 bounds;
    const ch_augment_desc &d = desc[blockIdx.x];
    const int y = blockIdx.y, nw = d.nw;
    if (d.nrows == 0 || y >= d.nh) return;   // block-uniform
    if (threadIdx.x == 0) bounds = bilinear_coeffs(d.h, d.nh, y, kk, 1);
    __syncthreads();
    const int ymin = bounds.x - d.row0, n = bounds.y;
    const uint8_t *tmp = ws + d.tmp_offset + (size_t)ymin * nw * 3;
    uint8_t *img = ws + d.img_offset + (size_t)y * nw * 3;
    for (int x = threadIdx.x; x < nw; x += 256) {
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int k = kk[t];
            const uint8_t *p = tmp + ((size_t)t * nw + x) * 3;
            a0 += (int)p[0] * k;
            a1 += (int)p[1] * k;
            a2 += (int)p[2] * k;
        }
        uint8_t *o = img + (size_t)(d.flip ? nw - 1 - x : x) * 3;
        o[0] = (uint8_t)clip8(a0);
        o[1] = (uint8_t)clip8(a1);
        o[2] = (uint8_t)clip8(a2);
    }
}

// per-image table [channel][byte] for the ops that are one: histograms first where the op needs them
__global__ __launch_bounds__(256) void ta_lut_kernel(const ch_augment_desc *__restrict__ desc, uint8_t *__restrict__ ws) {
    __shared__ int hist[LUT_BYTES];
    __shared__ int mean_l;
    const ch_augment_desc &d = desc[blockIdx.x];
    const int op = d.op, tid = threadIdx.x;
    if (d.nrows == 0 || !uses_lut(op, d.iparam)) return;   // block-uniform
    uint8_t *lut = ws + (size_t)blockIdx.x * LUT_BYTES;
    const int64_t npix = (int64_t)d.nh * d.nw;
    if (op == OP_CONTRAST || op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
        for (int i = tid; i < LUT_BYTES; i += 256) hist[i] = 0;
        __syncthreads();
        const uint8_t *img = ws + d.img_offset;
        for (int64_t p = tid; p < npix; p += 256) {
            const int r = img[p * 3 + 0], g = img[p * 3 + 1], b = img[p * 3 + 2];
            if (op == OP_CONTRAST) {
                atomicAdd(&hist[rgb_to_l(r, g, b)], 1);
            } else {
                atomicAdd(&hist[r], 1);
                atomicAdd(&hist[256 + g], 1);
                atomicAdd(&hist[512 + b], 1);
            }
        }
        __syncthreads();
    }
    const float alpha = (float)d.fparam;
    if (op == OP_CONTRAST) {
        if (tid == 0) {   // ImageStat.Stat(L).mean[0]: sum of j * h[j] in doubles (exact: integers), / count; int(mean + 0.5)
            double sum = 0.0;
            for (int j = 0; j < 256; ++j) sum += (double)((int64_t)j * hist[j]);
            const double mean = sum / (double)npix;
            mean_l = (int)(mean + 0.5);
        }
        __syncthreads();
    }
    if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
        if (tid < 3) {    // one lane per channel: ImageOps' serial loops
            const int *h = hist + tid * 256;
            uint8_t *l = lut + tid * 256;
            int lo = 0, hi = 255, nz = 0;
            int64_t total = 0;
            while (lo < 255 && h[lo] == 0) ++lo;
            while (hi > 0 && h[hi] == 0) --hi;
            for (int i = 0; i < 256; ++i) {
                nz += h[i] != 0;
                total += h[i];
            }
            if (op == OP_AUTOCONTRAST) {
                if (hi <= lo) {
                    for (int i = 0; i < 256; ++i) l[i] = (uint8_t)i;
                } else {
                    const double scale = 255.0 / (hi - lo);
                    const double offset = -lo * scale;
                    for (int i = 0; i < 256; ++i) {
                        int ix = (int)(i * scale + offset);
                        l[i] = (uint8_t)(ix < 0 ? 0 : (ix > 255 ? 255 : ix));
                    }
                }
            } else {
                const int64_t step = nz <= 1 ? 0 : (total - h[hi]) / 255;
                if (step == 0) {
                    for (int i = 0; i < 256; ++i) l[i] = (uint8_t)i;
                } else {
                    int64_t n = step / 2;
                    for (int i = 0; i < 256; ++i) {
                        // Image.point clips a table entry to 255 (n / step reaches 256 at the last non-empty bin when the
                        // remainder of the step division is large)
                        l[i] = (uint8_t)min(n / step, (int64_t)255);
                        n += h[i];
                    }
                }
            }
        }
        return;
    }
    for (int i = tid; i < LUT_BYTES; i += 256) {
        const int v = i & 255;
        int o = v;
        if (op == OP_BRIGHTNESS) o = blend8(0, v, alpha);
        else if (op == OP_CONTRAST) o = blend8(mean_l, v, alpha);
        else if (op == OP_POSTERIZE) o = v & ~((1 << (8 - d.iparam)) - 1);
        else if (op == OP_SOLARIZE) o = (double)v < d.fparam ? v : 255 - v;
        lut[i] = (uint8_t)o;
    }
}

// Pillow's BICUBIC macro (Geometry.c): a = -1 cubic convolution in double
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// Image.transform(size, AFFINE, m, BICUBIC, fillcolor=0) at output pixel (X, Y): affine_transform + bicubic_filter32RGB
__device__ __forceinline__ void affine_bicubic(const uint8_t *img, int W, int H, const double *m, int X, int Y, int v[3]) {
    const double xo = X + 0.5, yo = Y + 0.5;
    double xin = m[0] * xo + m[1] * yo + m[2];
    double yin = m[3] * xo + m[4] * yo + m[5];
    v[0] = v[1] = v[2] = 0;
    if (xin < 0.0 || xin >= W || yin < 0.0 || yin >= H) return;   // the fill colour
    xin -= 0.5;
    yin -= 0.5;
    int x = xin < 0.0 ? (int)floor(xin) : (int)xin;
    int y = yin < 0.0 ? (int)floor(yin) : (int)yin;
    const double dx = xin - x, dy = yin - y;
    --x;
    --y;
    int xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = min(max(x + k, 0), W - 1) * 3;
    int rows[4];
    rows[0] = min(max(y, 0), H - 1);
#pragma unroll
    for (int k = 1; k < 4; ++k) rows[k] = (y + k >= 0 && y + k < H) ? y + k : -1;   // -1: repeat the previous row's value
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        double vv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k > 0 && rows[k] < 0) {
                vv[k] = vv[k - 1];
            } else {
                const uint8_t *in = img + (size_t)rows[k] * W * 3 + b;
                vv[k] = cubic(in[xs[0]], in[xs[1]], in[xs[2]], in[xs[3]], dx);
            }
        }
        const double r = cubic(vv[0], vv[1], vv[2], vv[3], dy);
        v[b] = r <= 0.0 ? 0 : (r >= 255.0 ? 255 : (int)r);
    }
}

// the crop window of the augmented image -> ToTensor -> normalise: out[b][c][y][x]
template <typename OUT>
__global__ __launch_bounds__(256) void ta_output_kernel(const ch_augment_desc *__restrict__ desc, const uint8_t *__restrict__ ws, int crop,
                                                        float m0, float m1, float m2, float s0, float s1, float s2, OUT *__restrict__ out) {
    const ch_augment_desc &d = desc[blockIdx.x];
    const int y = blockIdx.y, x = threadIdx.x;
    if (d.nrows == 0 || x >= crop) return;
    const int W = d.nw, H = d.nh, X = x + d.left, Y = y + d.top, op = d.op, ip = d.iparam;
    const uint8_t *img = ws + d.img_offset;
    const uint8_t *p = img + ((size_t)Y * W + X) * 3;
    const float alpha = (float)d.fparam;
    int v[3];
    if (uses_lut(op, ip)) {
        const uint8_t *lut = ws + (size_t)blockIdx.x * LUT_BYTES;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = lut[c * 256 + p[c]];
    } else if (op == OP_COLOR) {
        const int l = rgb_to_l(p[0], p[1], p[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend8(l, p[c], alpha);
    } else if (op == OP_SHARPNESS) {
        // ImageFilter.SMOOTH (3x3, 1 1 1 / 1 5 1 / 1 1 1, scale 13): float kernel, rows y+1, y, y-1 summed row by row onto 0.5,
        // truncated and clipped; the image's first / last row and column are copied
        const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0);
        const bool border = X == 0 || Y == 0 || X == W - 1 || Y == H - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int deg = p[c];
            if (!border) {
                const uint8_t *rd = p + (size_t)W * 3, *ru = p - (size_t)W * 3;
                float s = 0.5f;
                s += (float)rd[c - 3] * k1 + (float)rd[c] * k1 + (float)rd[c + 3] * k1;
                s += (float)p[c - 3] * k1 + (float)p[c] * k5 + (float)p[c + 3] * k1;
                s += (float)ru[c - 3] * k1 + (float)ru[c] * k1 + (float)ru[c + 3] * k1;
                deg = s <= 0.0f ? 0 : (s >= 255.0f ? 255 : (int)s);
            }
            v[c] = blend8(deg, p[c], alpha);
        }
    } else if (op == OP_ROTATE && ip != ROT_AFFINE) {
        // Image.transpose on a square image (W == H): ROTATE_90 / ROTATE_270 / ROTATE_180
        const int sy = ip == ROT_90 ? X : (ip == ROT_270 ? H - 1 - X : H - 1 - Y);
        const int sx = ip == ROT_90 ? W - 1 - Y : (ip == ROT_270 ? Y : W - 1 - X);
        const uint8_t *q = img + ((size_t)sy * W + sx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = q[c];
    } else {
        affine_bicubic(img, W, H, d.m, X, Y, v);
    }
    const float v0 = ((float)v[0] / 255.0f - m0) / s0;
    const float v1 = ((float)v[1] / 255.0f - m1) / s1;
    const float v2 = ((float)v[2] / 255.0f - m2) / s2;
    const size_t plane = (size_t)crop * crop;
    OUT *o = out + (size_t)blockIdx.x * 3 * plane + (size_t)y * crop + x;
    if constexpr (sizeof(OUT) == 2) {
        o[0] = f2bf(v0);
        o[plane] = f2bf(v1);
        o[2 * plane] = f2bf(v2);
    } else {
        o[0] = v0;
        o[plane] = v1;
        o[2 * plane] = v2;
    }
}

}  // namespace

extern "C" int64_t ch_augment_workspace(int32_t B, int64_t image_bytes) {
    return round_up64((int64_t)(B > 0 ? B : 0) * LUT_BYTES, 256) + (image_bytes > 0 ? image_bytes : 0);
}

extern "C" int ch_preprocess_augment(const uint8_t *pixels, const ch_augment_desc *desc_device, int32_t B, int32_t max_rows, int32_t max_nh,
                                     int32_t max_nw, int32_t crop, const float *mean3_host, const float *std3_host, void *out,
                                     int32_t out_dtype, uint8_t *workspace, void *stream) {
    CH_REQUIRE(B >= 0 && crop >= 1 && crop <= 256, "preprocess_augment: crop must be in [1, 256]");
    if (B == 0) return 0;
    CH_REQUIRE(pixels && desc_device && mean3_host && std3_host && out && workspace, "preprocess_augment: null pointer");
    CH_REQUIRE(max_rows >= 1 && max_nh >= 1 && max_nw >= 1, "preprocess_augment: max_rows / max_nh / max_nw must be >= 1");
    CH_REQUIRE(out_dtype == 0 || out_dtype == 1, "preprocess_augment: out_dtype must be 0 (fp32) or 1 (bf16)");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ta_resize_h_kernel, dim3((unsigned)B, (unsigned)ceil_div64(max_rows, HROWS)), dim3(256), 0, s, pixels, desc_device,
                       workspace);
    CH_LAUNCH_CHECK();
    hipLaunchKernelGGL(ta_resize_v_kernel, dim3((unsigned)B, (unsigned)max_nh), dim3(256), 0, s, desc_device, workspace);
    CH_LAUNCH_CHECK();
    hipLaunchKernelGGL(ta_lut_kernel, dim3((unsigned)B), dim3(256), 0, s, desc_device, workspace);
    CH_LAUNCH_CHECK();
    const float *m = mean3_host, *sd = std3_host;
    const dim3 grid((unsigned)B, (unsigned)crop), block(256);
    if (out_dtype == 1)
        hipLaunchKernelGGL(ta_output_kernel<bf16_t>, grid, block, 0, s, desc_device, workspace, crop, m[0], m[1], m[2], sd[0], sd[1], sd[2],
                           (bf16_t *)out);
    else
        hipLaunchKernelGGL(ta_output_kernel<float>, grid, block, 0, s, desc_device, workspace, crop, m[0], m[1], m[2], sd[0], sd[1], sd[2],
                           (float *)out);
    CH_LAUNCH_CHECK();
    return 0;
}
