// Region-wise makeup transfer from several references (BUILD-DEFINED): the spatial blend of R <= 8 ControlNet hint
// embeddings and the kernel that makes its weights from region masks.
//
//   E[b, p, :] = sum_r w[b, r, p] * E_r[b, p, :]      acc = w0 e0, then acc = fma(w_r, e_r, acc) for r = 1, 2, ... in fp32, ONE bf16 rounding
//
// Weights from masks [K][B][H][W] (K = R - 1): a pixel belongs to the lowest k whose mask is non-zero; cnt_k = owned pixels of a
// factor x factor block; S_k = sum of cnt_k over the (2 feather + 1)^2 window with clamp-to-edge indices (an integer);
// a_k = float(S_k) / float((2 feather + 1)^2 factor^2); w_{k+1} = strength[b, k] * a_k; w_0 = max(0, ((1 - w_1) - w_2) - ...).  Every
// fp32 operation is an explicit correctly rounded intrinsic (-ffp-contract must not fuse strength * a into the subtraction), so the
// output has the bits of a numpy float32 restatement.
//
// Pixel-space background paste after the decode (reference Fixbackground.get_target, diffmk/makeup_teacher.py:254-262; the feather is
// BUILD-DEFINED): out = clamp((a (s + 1) / 2 + (1 - a) (t + 1) / 2) 2 - 1, -1, 1) over fp32 NCHW, a = the keep weight of a pixel, either
// the region_weights rule at pixel resolution over a label map (integer window sums, one division) or an fp32 mask read as is.  One
// launch: 256 threads cover a tile of PB_TH = 16 rows x PB_TW = 64 columns, 4 consecutive pixels of one row per thread; grid
// (ceil(W / 64) * ceil(H / 16), B), tiles row-major in x.  Seven explicit correctly rounded operations per element, as above.
#include "mkd_common.h"

namespace {

constexpr int RG_MAX = 8;                       // references per blend
constexpr int RG_LDS_COUNTS = 32768;            // uint16 block counts of one sample that fit 64 KiB of LDS: K * h * w

struct RegionPtrs { const bf16_t* e[RG_MAX]; };

// one lane = 8 channels of one pixel: R 16-byte loads, one 16-byte store; the pixel's R weights are one load each (the lanes of a
// pixel read the same address).  No __restrict__ on the embeddings: out may be e[0] (every lane reads its own 16 bytes before it writes them)
__global__ __launch_bounds__(256) void region_blend_kernel(const RegionPtrs ptrs, const float* __restrict__ weights, bf16_t* out,
                                                           int64_t total, int hw, int C8, int R) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = idx / C8;                       // b * hw + p
        const int64_t b = pix / hw;
        const int p = (int)(pix - b * hw);
        const float* wp = weights + b * R * hw + p;
        float acc[8];
        {
            const float w0 = wp[0];
            const U16x8 v = *(const U16x8*)(ptrs.e[0] + idx * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __fmul_rn(w0, bf16_to_f32(v.v[j]));
        }
#pragma unroll
        for (int r = 1; r < RG_MAX; ++r) {                  // unrolled with static table indices: the by-value table stays in SGPRs
            if (r < R) {
                const float wr = wp[(int64_t)r * hw];
                const U16x8 v = *(const U16x8*)(ptrs.e[r] + idx * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = __fmaf_rn(wr, bf16_to_f32(v.v[j]), acc[j]);
            }
        }
        U16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = f32_to_bf16(acc[j]);
        *(U16x8*)(out + idx * 8) = o;
    }
}

// One workgroup per sample.  Phase 1: every thread counts the owned pixels of whole factor x factor blocks into LDS
// (cnt[k][h * w] uint16: a count is <= 64^2); phase 2: window sums from LDS and the weights.  VEC4: 4 mask bytes per load
// (factor % 4 == 0 and a 4-byte aligned base make every block row 4-byte aligned).
template <bool VEC4>
__global__ __launch_bounds__(256) void region_weights_kernel(const uint8_t* __restrict__ masks, int K, int B, int H, int W, int f, int rho,
                                                             const float* __restrict__ strength, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rg_smem[];
    uint16_t* cnt = (uint16_t*)rg_smem;
    const int b = blockIdx.x;
    const int h = H / f, w = W / f, hw = h * w;
    const size_t plane = (size_t)B * H * W;                 // mask k of sample b: masks + k * plane + b * H * W
    const uint8_t* mb = masks + (size_t)b * H * W;
    for (int o = threadIdx.x; o < hw; o += blockDim.x) {
        const int y = o / w, x = o - y * w;
        const uint8_t* src = mb + ((size_t)y * f) * W + (size_t)x * f;
        int c[RG_MAX - 1];
#pragma unroll
        for (int k = 0; k < RG_MAX - 1; ++k) c[k] = 0;
        for (int dy = 0; dy < f; ++dy) {
            const uint8_t* row = src + (size_t)dy * W;
            if (VEC4) {
                for (int dx = 0; dx < f; dx += 4) {
                    uint32_t owned = 0;                     // per byte lane: 0x01 once a lower mask has claimed the pixel
#pragma unroll
                    for (int k = 0; k < RG_MAX - 1; ++k) {
                        if (k < K) {
                            const uint32_t v = *(const uint32_t*)(row + k * plane + dx);
                            // byte != 0 -> 0x01 in that byte (no carries across bytes: (v & 0x7f) + 0x7f <= 0xfe)
                            const uint32_t nz = ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) >> 7) & 0x01010101u;
                            c[k] += __popc(nz & ~owned);
                            owned |= nz;
                        }
                    }
                }
            } else {
                for (int dx = 0; dx < f; ++dx) {
                    bool owned = false;
#pragma unroll
                    for (int k = 0; k < RG_MAX - 1; ++k) {
                        if (k < K) {
                            const bool nz = row[k * plane + dx] != 0;
                            c[k] += (nz && !owned) ? 1 : 0;
                            owned = owned || nz;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RG_MAX - 1; ++k)
            if (k < K) cnt[k * hw + o] = (uint16_t)c[k];
    }
    __syncthreads();
    const int win = 2 * rho + 1;
    const float D = (float)(win * win * f * f);             // <= 81 * 4096: exact
    float* ob = out + (size_t)b * (K + 1) * hw;
    for (int o = threadIdx.x; o < hw; o += blockDim.x) {
        const int y = o / w, x = o - y * w;
        float rem = 1.0f;
        for (int k = 0; k < K; ++k) {
            const uint16_t* ck = cnt + k * hw;
            int S = 0;
            for (int dy = -rho; dy <= rho; ++dy) {
                const int yy = min(max(y + dy, 0), h - 1);
                for (int dx = -rho; dx <= rho; ++dx) S += ck[yy * w + min(max(x + dx, 0), w - 1)];
            }
            const float a = __fdiv_rn((float)S, D);
            const float wk = strength ? __fmul_rn(strength[b * K + k], a) : a;
            ob[(size_t)(k + 1) * hw + o] = wk;
            rem = __fsub_rn(rem, wk);
        }
        ob[o] = fmaxf(0.0f, rem);
    }
}

constexpr int PB_TH = 16, PB_TW = 64;           // paste tile: rows x columns of 256 threads, 4 consecutive pixels of a row each
constexpr int PB_MAX_FEATHER = 16;

// the reference's expression, one rounding per operation: u = (s + 1) / 2, v = (t + 1) / 2, r = a u + (1 - a) v, o = clamp(r 2 - 1)
// (x / 2 and x * 0.5 are the same real number, so the same fp32); every product that feeds an addition is a mkd_rounded (mkd_common.h)
__device__ __forceinline__ float pb_paste(float a, float s, float t) {
    const float u = __fmul_rn(__fadd_rn(s, 1.0f), 0.5f);
    const float v = __fmul_rn(__fadd_rn(t, 1.0f), 0.5f);
    const float p = mkd_rounded(__fmul_rn(a, u));
    const float q = mkd_rounded(__fmul_rn(__fsub_rn(1.0f, a), v));
    const float r = __fadd_rn(p, q);
    const float o = __fsub_rn(mkd_rounded(__fmul_rn(r, 2.0f)), 1.0f);
    return fminf(fmaxf(o, -1.0f), 1.0f);
}

// LABELS: the keep weight comes from the label map.  Phase 1 stages cnt (in-class label pixels of an f x f block) of the tile plus a
// halo of rho as uint16 [(16 + 2 rho)][(64 + 2 rho)], entry (ly, lx) = image pixel (clamp(y0 - rho + ly), clamp(x0 - rho + lx)), so the
// clamp-to-edge rule is applied once, here; phase 2 takes horizontal window sums into uint32 [(16 + 2 rho)][64]; phase 3 sums 2 rho + 1
// rows of those per output pixel (16-byte LDS reads: 4 pixels).  !LABELS: a = mask[b or 0][y][x], no LDS, no barrier (uniform over
// the launch).  VEC: W % 4 == 0 and 16-byte aligned pointers, so a thread's 4 pixels are one 16-byte access and all inside or all
// outside the image; otherwise pixel by pixel with the same arithmetic.  No __restrict__ on image / out: out may be image (every
// thread reads its own elements before it writes them).
template <bool LABELS, bool VEC>
__global__ __launch_bounds__(256) void paste_background_kernel(const float* image, const float* __restrict__ src,
                                                               const uint8_t* __restrict__ labels, unsigned long long classes, int f, int rho,
                                                               const float* __restrict__ mask, int mask_batch, float* out,
                                                               float* __restrict__ alpha_out, int C, int H, int W, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_smem[];
    const int b = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * PB_TH, x0 = tx * PB_TW;
    const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
    const int y = y0 + r, x = x0 + c4;
    const size_t hw = (size_t)H * W;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (LABELS) {
        const int cw = PB_TW + 2 * rho, ch = PB_TH + 2 * rho;
        uint32_t* hs = (uint32_t*)pb_smem;                                  // [ch][64], first: its rows stay 16-byte aligned
        uint16_t* cnt = (uint16_t*)(pb_smem + (size_t)ch * PB_TW * sizeof(uint32_t));       // [ch][cw]
        const size_t LW = (size_t)W * f;
        const uint8_t* lb = labels + (size_t)b * hw * f * f;
        for (int e = threadIdx.x; e < ch * cw; e += 256) {
            const int ly = e / cw, lx = e - ly * cw;
            const int py = min(max(y0 - rho + ly, 0), H - 1), px = min(max(x0 - rho + lx, 0), W - 1);
            const uint8_t* blk = lb + (size_t)py * f * LW + (size_t)px * f;
            int n = 0;
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) {
                    const unsigned l = blk[dy * LW + dx];
                    n += (l < 64u && ((classes >> l) & 1ull)) ? 1 : 0;
                }
            cnt[e] = (uint16_t)n;
        }
        __syncthreads();
        const int win = 2 * rho + 1;
        for (int e = threadIdx.x; e < ch * PB_TW; e += 256) {
            const int ly = e >> 6, lx = e & 63;
            const uint16_t* row = cnt + ly * cw + lx;
            uint32_t s = 0;
            for (int d = 0; d < win; ++d) s += row[d];
            hs[e] = s;
        }
        __syncthreads();
        uint32_t S[4] = {0u, 0u, 0u, 0u};
        for (int d = 0; d < win; ++d) {
            const uint4 v = *(const uint4*)(hs + (r + d) * PB_TW + c4);
            S[0] += v.x; S[1] += v.y; S[2] += v.z; S[3] += v.w;
        }
        const float D = (float)(win * win * f * f);                         // <= 33^2 * 64 = 69696: exact, and so is every S
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = __fdiv_rn((float)S[j], D);
    }
    if (y >= H || x >= W) return;                                           // (after the last barrier)
    const size_t pix = (size_t)y * W + x;
    if (VEC) {
        if (!LABELS) {
            const float4 m = *(const float4*)(mask + (mask_batch == 1 ? 0 : (size_t)b * hw) + pix);
            a[0] = m.x; a[1] = m.y; a[2] = m.z; a[3] = m.w;
        }
        if (alpha_out) *(float4*)(alpha_out + (size_t)b * hw + pix) = make_float4(a[0], a[1], a[2], a[3]);
        for (int c = 0; c < C; ++c) {
            const size_t o = ((size_t)b * C + c) * hw + pix;
            const float4 s = *(const float4*)(src + o);
            const float4 t = *(const float4*)(image + o);
            *(float4*)(out + o) = make_float4(pb_paste(a[0], s.x, t.x), pb_paste(a[1], s.y, t.y), pb_paste(a[2], s.z, t.z),
                                              pb_paste(a[3], s.w, t.w));
        }
    } else {
        const int n = min(4, W - x);
        if (!LABELS) {
            const float* mp = mask + (mask_batch == 1 ? 0 : (size_t)b * hw) + pix;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) a[j] = mp[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (alpha_out && j < n) alpha_out[(size_t)b * hw + pix + j] = a[j];
        for (int c = 0; c < C; ++c) {
            const size_t o = ((size_t)b * C + c) * hw + pix;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) out[o + j] = pb_paste(a[j], src[o + j], image[o + j]);
        }
    }
}

inline int rg_grid_for(int64_t total, int block = 256, int cap = 4096) {
    const int64_t g = (total + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

int launch_region_blend(const bf16_t* const* e, const float* weights, bf16_t* out, int batch, int hw, int C, int R, hipStream_t stream) {
    if (!e || !weights || !out || batch <= 0 || hw <= 0 || C <= 0 || C % 8 || R < 1 || R > RG_MAX)
        return mkd_fail(-1, "region_blend: R in 1..8 bf16 [B, hw, C] embeddings with C a multiple of 8, weights [B, R, hw]");
    RegionPtrs p;
    for (int r = 0; r < RG_MAX; ++r) {
        p.e[r] = r < R ? e[r] : nullptr;
        if (r < R && (!e[r] || ((uintptr_t)e[r] & 15))) return mkd_fail(-1, "region_blend: every embedding must be a 16-byte aligned device pointer");
    }
    if ((uintptr_t)out & 15) return mkd_fail(-1, "region_blend: out must be 16-byte aligned");
    const int64_t total = (int64_t)batch * hw * (C / 8);
    hipLaunchKernelGGL(region_blend_kernel, dim3(rg_grid_for(total)), dim3(256), 0, stream, p, weights, out, total, hw, C / 8, R);
    MKD_LAUNCH_CHECK("region_blend_kernel");
    return 0;
}

int launch_region_weights(const uint8_t* masks, int n_masks, int batch, int H, int W, int f, int feather, const float* strength, float* out,
                          hipStream_t stream) {
    if (!masks || !out || n_masks < 1 || n_masks > RG_MAX - 1 || batch <= 0 || batch > 65535 || f < 1 || f > 64 || H < f || W < f || H % f || W % f)
        return mkd_fail(-1, "region_weights: masks [K, B, H, W] with K in 1..7 and H, W positive multiples of the factor (1..64)");
    if (feather < 0 || feather > 4) return mkd_fail(-1, "region_weights: feather must be 0..4 latent pixels");
    const int64_t counts = (int64_t)n_masks * (H / f) * (W / f);
    if (counts > RG_LDS_COUNTS)
        return mkd_fail(-1, "region_weights: K * (H / factor) * (W / factor) must not exceed 32768 (the block counts of a sample are staged in LDS)");
    const size_t lds = ((size_t)counts * sizeof(uint16_t) + 15) & ~(size_t)15;
    if (f % 4 == 0 && ((uintptr_t)masks & 3) == 0)
        hipLaunchKernelGGL(region_weights_kernel<true>, dim3(batch), dim3(256), lds, stream, masks, n_masks, batch, H, W, f, feather, strength, out);
    else
        hipLaunchKernelGGL(region_weights_kernel<false>, dim3(batch), dim3(256), lds, stream, masks, n_masks, batch, H, W, f, feather, strength, out);
    MKD_LAUNCH_CHECK("region_weights_kernel");
    return 0;
}

int launch_paste_background(const float* image, const float* src, const uint8_t* labels, uint64_t classes, int f, int feather, const float* mask,
                            int mask_batch, float* out, float* alpha_out, int batch, int channels, int H, int W, hipStream_t stream) {
    if (!image || !src || !out) return mkd_fail(-1, "paste_background: null image / src / out");
    if ((labels != nullptr) == (mask != nullptr)) return mkd_fail(-1, "paste_background: exactly one of labels and mask must be given");
    if (batch < 1 || batch > 65535 || channels < 1 || channels > 8 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 24)
        return mkd_fail(-1, "paste_background: batch 1..65535, channels 1..8, H, W >= 1 and H * W <= 2^24");
    if (labels && (f < 1 || f > 8)) return mkd_fail(-1, "paste_background: factor must be 1..8");
    if (feather < 0 || feather > PB_MAX_FEATHER || (mask && feather)) return mkd_fail(-1, "paste_background: feather must be 0..16, and 0 with a mask");
    if (mask && mask_batch != 1 && mask_batch != batch) return mkd_fail(-1, "paste_background: mask_batch must be 1 or batch");
    const int tiles_x = (W + PB_TW - 1) / PB_TW, tiles_y = (H + PB_TH - 1) / PB_TH;
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)batch);             // <= 2^24 / 16 tiles in x
    const uintptr_t al = (uintptr_t)image | (uintptr_t)src | (uintptr_t)out | (uintptr_t)alpha_out | (uintptr_t)mask;
    const bool vec = W % 4 == 0 && (al & 15) == 0;
    if (labels) {
        const int ch = PB_TH + 2 * feather, cw = PB_TW + 2 * feather;
        const size_t lds = ((size_t)ch * PB_TW * sizeof(uint32_t) + (size_t)ch * cw * sizeof(uint16_t) + 15) & ~(size_t)15;     // <= 21504
        if (vec)
            hipLaunchKernelGGL((paste_background_kernel<true, true>), grid, dim3(256), lds, stream, image, src, labels, (unsigned long long)classes,
                               f, feather, mask, mask_batch, out, alpha_out, channels, H, W, tiles_x);
        else
            hipLaunchKernelGGL((paste_background_kernel<true, false>), grid, dim3(256), lds, stream, image, src, labels, (unsigned long long)classes,
                               f, feather, mask, mask_batch, out, alpha_out, channels, H, W, tiles_x);
    } else if (vec) {
        hipLaunchKernelGGL((paste_background_kernel<false, true>), grid, dim3(256), 0, stream, image, src, labels, (unsigned long long)classes, f,
                           feather, mask, mask_batch, out, alpha_out, channels, H, W, tiles_x);
    } else {
        hipLaunchKernelGGL((paste_background_kernel<false, false>), grid, dim3(256), 0, stream, image, src, labels, (unsigned long long)classes, f,
                           feather, mask, mask_batch, out, alpha_out, channels, H, W, tiles_x);
    }
    MKD_LAUNCH_CHECK("paste_background_kernel");
    return 0;
}
