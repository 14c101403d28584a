// Kernels of the face-parsing network (BiSeNet, ResNet-18 context path) that are not convolutions on the implicit-GEMM kernels:
// the stem (normalise + 7x7 stride-2 convolution + folded BN + ReLU, then the 3x3 stride-2 max-pool), the channel gates (global mean +
// one or two small mat-vecs), the gate apply, the stride-2 row gather in front of the 1x1 shortcuts, and the head (bilinear
// upsample + argmax + class remap without an H x W x classes tensor).  UPSTREAM: zllrunning/face-parsing.PyTorch model.py / resnet.py.
// No atomics, no inter-workgroup hand-offs; every reduction runs in a fixed order.
#include "mkd_common.h"
#include "parser.h"

namespace {

// The library is built with -ffp-contract=fast; where the ABI promises separately rounded operations the product goes through this
// before it meets its addition, so the two cannot become one fma.
__device__ __forceinline__ float rounded(float v) { asm volatile("" : "+v"(v)); return v; }

constexpr int STEM_T = 8;                          // output tile of the stem convolution: 8 x 8 pixels at H/2
constexpr int STEM_P = 2 * STEM_T + 5;             // its input patch: 21 x 21
constexpr int STEM_TAPS = 147;                     // 7 * 7 * 3

// ---- stem, launch 1: x fp32 NCHW [B,3,H,W] in [0,1] -> y bf16 NHWC [B,H/2,W/2,C0] = relu(conv7x7_s2_p3((x - mean) / std) + bias) -----------
// One workgroup per 8 x 8 output tile.  The NORMALISED patch sits in LDS with zeros outside the image (the padding applies to the
// normalised image, so the constants cannot move into the bias); the weights sit in LDS as bf16 [tap][C0], tap = (ky * 7 + kx) * 3 + c.
// Thread (pixel = tid & 63, group = tid >> 6) owns 8 channels of a pixel per pass: the 64 lanes of a wave read the same weights
// (LDS broadcast) and different patch words.
__global__ __launch_bounds__(256) void parser_stem_conv_kernel(const float* __restrict__ x, const bf16_t* __restrict__ w, const float* __restrict__ bias,
                                                               bf16_t* __restrict__ y, int H, int W, int C0, float m0, float m1, float m2,
                                                               float s0, float s1, float s2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* const wl = (bf16_t*)smem;                                   // [147][C0]
    float* const patch = (float*)(smem + (size_t)STEM_TAPS * C0 * 2);    // [3][21][21]   (147 * C0 * 2 is a multiple of 16: C0 % 8 == 0)
    const int tid = threadIdx.x;
    const int H2 = H >> 1, W2 = W >> 1;
    const int ox0 = blockIdx.x * STEM_T, oy0 = blockIdx.y * STEM_T, b = blockIdx.z;
    for (int i = tid; i < STEM_TAPS * C0 / 8; i += 256) ((U16x8*)wl)[i] = ((const U16x8*)w)[i];
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
    for (int i = tid; i < 3 * STEM_P * STEM_P; i += 256) {
        const int c = i / (STEM_P * STEM_P), r = i - c * STEM_P * STEM_P;
        const int py = r / STEM_P, px = r - py * STEM_P;
        const int iy = iy0 + py, ix = ix0 + px;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
            v = (x[(((size_t)b * 3 + c) * H + iy) * W + ix] - mean) / sd;
        }
        patch[i] = v;
    }
    __syncthreads();
    const int pix = tid & 63, py = pix >> 3, px = pix & 7;
    const int oy = oy0 + py, ox = ox0 + px;
    for (int g = tid >> 6; g < C0 / 8; g += 4) {
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int ky = 0; ky < 7; ++ky)
            for (int kx = 0; kx < 7; ++kx) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = patch[(c * STEM_P + 2 * py + ky) * STEM_P + 2 * px + kx];
                    const U16x8 wv = *(const U16x8*)(wl + (size_t)((ky * 7 + kx) * 3 + c) * C0 + g * 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(v, bf16_to_f32(wv.v[j]), acc[j]);
                }
            }
        if (oy < H2 && ox < W2) {
            U16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = f32_to_bf16(fmaxf(acc[j] + bias[g * 8 + j], 0.f));
            *(U16x8*)(y + (((size_t)b * H2 + oy) * W2 + ox) * C0 + g * 8) = o;
        }
    }
}

// ---- stem, launch 2: 3x3 stride-2 pad-1 max-pool over bf16 NHWC; taps outside the image are ignored ------------------------------------
__global__ __launch_bounds__(256) void parser_maxpool_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int batch, int Hin, int Win, int C) {
    const int G = C / 8, Ho = Hin >> 1, Wo = Win >> 1;
    const size_t n = (size_t)batch * Ho * Wo * G;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = (int)(i % G);
    size_t p = i / G;
    const int ox = (int)(p % Wo); p /= Wo;
    const int oy = (int)(p % Ho);
    const int b = (int)(p / Ho);
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    for (int dy = -1; dy <= 1; ++dy) {
        const int iy = 2 * oy + dy;
        if (iy < 0 || iy >= Hin) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int ix = 2 * ox + dx;
            if (ix < 0 || ix >= Win) continue;
            const U16x8 v = *(const U16x8*)(x + (((size_t)b * Hin + iy) * Win + ix) * C + g * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], bf16_to_f32(v.v[j]));
        }
    }
    U16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = f32_to_bf16(m[j]);
    *(U16x8*)(y + (((size_t)b * Ho + oy) * Wo + ox) * C + g * 8) = o;
}

// ---- row gather in front of a stride-2 1x1 shortcut: y[b, oy, ox, :] = x[b, 2 oy, 2 ox, :] ----------------------------------------------
__global__ __launch_bounds__(256) void parser_subsample_kernel(const bf16_t* __restrict__ x, int ldx, bf16_t* __restrict__ y, int batch, int Hin, int Win, int C) {
    const int G = C / 8, Ho = Hin >> 1, Wo = Win >> 1;
    const size_t n = (size_t)batch * Ho * Wo * G;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = (int)(i % G);
    size_t p = i / G;
    const int ox = (int)(p % Wo); p /= Wo;
    const int oy = (int)(p % Ho);
    const int b = (int)(p / Ho);
    *(U16x8*)(y + (((size_t)b * Ho + oy) * Wo + ox) * C + g * 8) = *(const U16x8*)(x + (((size_t)b * Hin + 2 * oy) * Win + 2 * ox) * ldx + g * 8);
}

// ---- channel gate: one workgroup per sample ---------------------------------------------------------------------------------------------
// mean[c] over the sample's pixels in fp32: thread (slice s, channel group g) adds pixels s, s + S, ... in order, the S partials of a
// channel are added in order s = 0 .. S - 1, then one division.  S depends on C alone, so the bits depend on nothing but the sample.
// Then h = act1(W1 mean + b1) and, when W2 is given, out = act2(W2 h + b2): one wave per output, lane l adds columns l, l + 64, ...,
// then a fixed xor tree.  act: 0 none, 1 ReLU, 2 1 / (1 + expf(-x)).
__device__ __forceinline__ float gate_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return 1.0f / (1.0f + expf(-v));
    return v;
}
__device__ __forceinline__ void gate_matvec(const float* __restrict__ w, const float* __restrict__ b, const float* in, int n_in, int n_out, int act,
                                            float* out, int tid) {
    const int lane = tid & 63;
    for (int j = tid >> 6; j < n_out; j += 4) {
        float a = 0.f;
        for (int c = lane; c < n_in; c += 64) a = fmaf(w[(size_t)j * n_in + c], in[c], a);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) out[j] = gate_act(a + (b ? b[j] : 0.f), act);
    }
}
__global__ __launch_bounds__(256) void parser_gate_kernel(const bf16_t* __restrict__ x, int ldx, int pixels, int C, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, int n1, int act1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, int n2, int act2, float* __restrict__ out) {
    __shared__ float part[2048];       // [S][C], S * C <= 256 * 8
    __shared__ float mean[PARSER_GATE_MAX];
    __shared__ float h1[PARSER_GATE_MAX];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int G = C / 8, S = 256 / G;
    const bf16_t* const xb = x + (size_t)b * pixels * ldx;
    if (tid < G * S) {
        const int g = tid % G, s = tid / G;
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = 0.f;
        for (int p = s; p < pixels; p += S) {
            const U16x8 v = *(const U16x8*)(xb + (size_t)p * ldx + g * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] += bf16_to_f32(v.v[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) part[s * C + g * 8 + j] = a[j];
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float a = 0.f;
        for (int s = 0; s < S; ++s) a += part[s * C + c];
        mean[c] = a / (float)pixels;
    }
    __syncthreads();
    float* const o = out + (size_t)b * (w2 ? n2 : n1);
    if (!w2) { gate_matvec(w1, b1, mean, C, n1, act1, o, tid); return; }
    gate_matvec(w1, b1, mean, C, n1, act1, h1, tid);
    __syncthreads();
    gate_matvec(w2, b2, h1, n1, n2, act2, o, tid);
}

// ---- gate apply: y[b, Y, X, c] = bf16(float(x[b, Y >> u, X >> u, c]) * a[b, c] + add) ---------------------------------------------------
// mode 0: add = v[b, c] (fp32); 1: add = r[b, Y >> u, X >> u, c] (bf16, pixel stride ldr); 2: add = x itself.  One fp32 product and one
// fp32 sum (never contracted), one bf16 rounding; 16-byte accesses.
__global__ __launch_bounds__(256) void parser_gate_apply_kernel(const bf16_t* __restrict__ x, int ldx, const float* __restrict__ a, int mode,
                                                                const float* __restrict__ v, const bf16_t* __restrict__ r, int ldr,
                                                                bf16_t* __restrict__ y, int ldy, int batch, int h, int w, int C, int u) {
    const int G = C / 8, Ho = h << u, Wo = w << u;
    const size_t n = (size_t)batch * Ho * Wo * G;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = (int)(i % G);
    size_t p = i / G;
    const int X = (int)(p % Wo); p /= Wo;
    const int Y = (int)(p % Ho);
    const int b = (int)(p / Ho);
    const size_t src = ((size_t)b * h + (Y >> u)) * w + (X >> u);
    const U16x8 xv = *(const U16x8*)(x + src * ldx + g * 8);
    const float* const ab = a + (size_t)b * C + g * 8;
    const f32x4 a0 = *(const f32x4*)ab, a1 = *(const f32x4*)(ab + 4);
    float add[8];
    if (mode == 0) {
        const float* const vb = v + (size_t)b * C + g * 8;
        const f32x4 v0 = *(const f32x4*)vb, v1 = *(const f32x4*)(vb + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { add[j] = v0[j]; add[4 + j] = v1[j]; }
    } else if (mode == 1) {
        const U16x8 rv = *(const U16x8*)(r + src * ldr + g * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) add[j] = bf16_to_f32(rv.v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) add[j] = bf16_to_f32(xv.v[j]);
    }
    U16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = f32_to_bf16(rounded(bf16_to_f32(xv.v[j]) * (j < 4 ? a0[j] : a1[j - 4])) + add[j]);
    *(U16x8*)(y + (((size_t)b * Ho + Y) * Wo + X) * ldy + g * 8) = o;
}

// ---- head: labels[b, oy, ox] = lut[argmax_c bilinear(logits[b, c])(py, px)], (py, px) = the nearest parse-resolution pixel ---------------
// The arithmetic (include/mkd.h: mkd_parse_labels) is one correctly rounded fp32 operation per step, nothing contracted.
struct HeadLut { uint8_t v[32]; };
__global__ __launch_bounds__(256) void parser_head_kernel(const float* __restrict__ logits, long long s_class, long long s_row, long long s_col,
                                                          long long s_batch, int n_classes, int h8, int w8, int P_h, int P_w, int out_h, int out_w,
                                                          float ry, float rx, int use_lut, HeadLut lut, uint8_t* __restrict__ labels) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, b = blockIdx.z;
    if (ox >= out_w) return;
    const int py = (int)(((long long)oy * P_h) / out_h), px = (int)(((long long)ox * P_w) / out_w);
    const float fy = rounded((float)py * ry), fx = rounded((float)px * rx);
    const int y0 = min((int)fy, h8 - 1), y1 = min(y0 + 1, h8 - 1);
    const int x0 = min((int)fx, w8 - 1), x1 = min(x0 + 1, w8 - 1);
    const float wy = fy - (float)y0, wx = fx - (float)x0;
    const float* const base = logits + (long long)b * s_batch;
    const long long o00 = y0 * s_row + x0 * s_col, o01 = y0 * s_row + x1 * s_col, o10 = y1 * s_row + x0 * s_col, o11 = y1 * s_row + x1 * s_col;
    float best = 0.f;
    int arg = 0;
    for (int c = 0; c < n_classes; ++c) {
        const float* const pc = base + c * s_class;
        const float v00 = pc[o00], v01 = pc[o01], v10 = pc[o10], v11 = pc[o11];
        const float top = v00 + rounded(wx * (v01 - v00));
        const float bot = v10 + rounded(wx * (v11 - v10));
        const float val = top + rounded(wy * (bot - top));
        if (c == 0 || val > best) { best = val; arg = c; }
    }
    labels[((size_t)b * out_h + oy) * out_w + ox] = use_lut ? lut.v[arg] : (uint8_t)arg;
}

// ---- logits fp32 NHWC (ld columns per pixel) -> NCHW [B, n_classes, h, w] ---------------------------------------------------------------
__global__ __launch_bounds__(256) void parser_logits_nchw_kernel(const float* __restrict__ x, int ld, float* __restrict__ y, int batch, int hw, int n_classes) {
    const size_t n = (size_t)batch * n_classes * hw;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = (int)(i % hw);
    const size_t q = i / hw;
    const int c = (int)(q % n_classes);
    const size_t b = q / n_classes;
    y[i] = x[(b * hw + p) * ld + c];
}

}  // namespace

static inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

size_t parser_stem_lds_bytes(int C0) { return (size_t)STEM_TAPS * C0 * 2 + (size_t)3 * STEM_P * STEM_P * 4; }

int launch_parser_stem_conv(const float* x, const bf16_t* w, const float* bias, bf16_t* y, int batch, int H, int W, int C0, const float* mean,
                            const float* stdv, hipStream_t stream) {
    const dim3 grid((W / 2) / STEM_T, (H / 2) / STEM_T, batch);
    hipLaunchKernelGGL(parser_stem_conv_kernel, grid, dim3(256), parser_stem_lds_bytes(C0), stream, x, w, bias, y, H, W, C0, mean[0], mean[1], mean[2],
                       stdv[0], stdv[1], stdv[2]);
    MKD_LAUNCH_CHECK("parser_stem_conv_kernel");
    return 0;
}
int launch_parser_maxpool(const bf16_t* x, bf16_t* y, int batch, int Hin, int Win, int C, hipStream_t stream) {
    const size_t n = (size_t)batch * (Hin / 2) * (Win / 2) * (C / 8);
    hipLaunchKernelGGL(parser_maxpool_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, x, y, batch, Hin, Win, C);
    MKD_LAUNCH_CHECK("parser_maxpool_kernel");
    return 0;
}
int launch_parser_subsample(const bf16_t* x, int ldx, bf16_t* y, int batch, int Hin, int Win, int C, hipStream_t stream) {
    const size_t n = (size_t)batch * (Hin / 2) * (Win / 2) * (C / 8);
    hipLaunchKernelGGL(parser_subsample_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, x, ldx, y, batch, Hin, Win, C);
    MKD_LAUNCH_CHECK("parser_subsample_kernel");
    return 0;
}
int launch_parser_gate(const bf16_t* x, int ldx, int batch, int pixels, int C, const float* w1, const float* b1, int n1, int act1, const float* w2,
                       const float* b2, int n2, int act2, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(parser_gate_kernel, dim3(batch), dim3(256), 0, stream, x, ldx, pixels, C, w1, b1, n1, act1, w2, b2, n2, act2, out);
    MKD_LAUNCH_CHECK("parser_gate_kernel");
    return 0;
}
int launch_parser_gate_apply(const bf16_t* x, int ldx, const float* a, int mode, const float* v, const bf16_t* r, int ldr, bf16_t* y, int ldy, int batch,
                             int h, int w, int C, int u, hipStream_t stream) {
    const size_t n = ((size_t)batch * (h << u) * (w << u)) * (C / 8);
    hipLaunchKernelGGL(parser_gate_apply_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, x, ldx, a, mode, v, r, ldr, y, ldy, batch, h, w, C, u);
    MKD_LAUNCH_CHECK("parser_gate_apply_kernel");
    return 0;
}
int launch_parser_head(const float* logits, int64_t s_class, int64_t s_row, int64_t s_col, int64_t s_batch, int batch, int n_classes, int h8, int w8,
                       int P_h, int P_w, int out_h, int out_w, const uint8_t* lut, uint8_t* labels, hipStream_t stream) {
    HeadLut t;
    for (int i = 0; i < 32; ++i) t.v[i] = (lut && i < n_classes) ? lut[i] : (uint8_t)i;
    const float ry = (h8 > 1 && P_h > 1) ? (float)(h8 - 1) / (float)(P_h - 1) : 0.f;
    const float rx = (w8 > 1 && P_w > 1) ? (float)(w8 - 1) / (float)(P_w - 1) : 0.f;
    const dim3 grid((out_w + 255) / 256, out_h, batch);
    hipLaunchKernelGGL(parser_head_kernel, grid, dim3(256), 0, stream, logits, (long long)s_class, (long long)s_row, (long long)s_col, (long long)s_batch,
                       n_classes, h8, w8, P_h, P_w, out_h, out_w, ry, rx, lut ? 1 : 0, t, labels);
    MKD_LAUNCH_CHECK("parser_head_kernel");
    return 0;
}
int launch_parser_logits_nchw(const float* x, int ld, float* y, int batch, int hw, int n_classes, hipStream_t stream) {
    const size_t n = (size_t)batch * n_classes * hw;
    hipLaunchKernelGGL(parser_logits_nchw_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, x, ld, y, batch, hw, n_classes);
    MKD_LAUNCH_CHECK("parser_logits_nchw_kernel");
    return 0;
}
