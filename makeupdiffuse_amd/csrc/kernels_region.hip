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
