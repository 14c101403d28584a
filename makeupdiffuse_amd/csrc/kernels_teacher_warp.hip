// The landmark-warped term of the teacher (mkd_pgt_warp; include/mkd.h holds the definition, tests/teacher_warp_ref.py restates it):
// EleGANt's AnnealingComposePGT (reference teacher.py:96-112) blends the reference, warped onto the source through the landmarks by a
// thin-plate spline, into the histogram-matched image xh.  BUILD-DEFINED: one spline per sample through all its control points.
//
//   s_k    = (y - c_ky)^2 + (x - c_kx)^2,  U(s) = s log(s) for s > 0, else 0
//   q_d    = ((sum_{k < K} w_dk U(s_k)) + a_d0) + a_d1 y + a_d2 x,  d in {y, x}: the position in the reference of source pixel p = (y, x)
//   m'_r   = the bilinear sample at q of "the reference's mask of region r is non-zero", a tap outside the image is 0
//   R_c    = the bilinear sample at q of clamp(ref_c, 0, 1) (NaN -> 0), tap indices clamped to the image
//   Wt     = min(1, sum_{r = 1..4} (alpha_r (c_r / Kw)) m'_r(q)),  c_r, Kw and the region ids as mkd_pgt_compose's, from the SOURCE masks
//   out_c  = float(xh_c + Wt (R_c - xh_c)); Wt = 0 gives the bits of xh_c
// all in double, every operation rounded on its own, the sums in the order written, ONE rounding to fp32.  NOTHING CONTRACTS: build.py
// compiles this file with -ffp-contract=off (under the library's -ffp-contract=fast the backend fuses a product into the next sum even
// below `#pragma clang fp contract(off)`, and a fused blend is off by one fp32 ulp about once in 2^29 values).
//
// One workgroup per 16 x 16 tile and a thread per pixel in every case: the K double logs of a pixel dwarf its three loads and stores, so
// there is no 16-byte form and no alignment can change the bits.  The sample's control points and coefficients sit in LDS as (y, x)
// pairs: every lane reads the same 16 bytes of each, a broadcast.  A tile whose counts are all zero copies xh and leaves before it
// stages them.
#include "mkd_common.h"
#include "pgt_regions.h"
#include "../../include/mkd.h"

namespace {

constexpr int PW_MAXK = 128;

struct PwPair { double y, x; };

// top = v00 + fx (v01 - v00), bot = v10 + fx (v11 - v10), v = top + fy (bot - top)
__device__ __forceinline__ double pw_bilinear(double v00, double v01, double v10, double v11, double fy, double fx) {
    const double top = v00 + fx * (v01 - v00);
    const double bot = v10 + fx * (v11 - v10);
    return top + fy * (bot - top);
}

__device__ __forceinline__ double pw_colour(float v) { return (double)(fminf(fmaxf(v, 0.0f), 1.0f) + 0.0f); }          // NaN -> 0, a zero is +0

// grid (tiles_x * tiles_y, n), 256 threads: thread 16 y + x is pixel (ty0 + y, tx0 + x).  xh and out may be the same array.
__global__ __launch_bounds__(256) void pgt_warp_kernel(const float* xh, const float* __restrict__ ref, const uint8_t* __restrict__ src_masks,
                                                       const uint8_t* __restrict__ ref_masks, const double* __restrict__ ctrl,
                                                       const double* __restrict__ coef, const int32_t* __restrict__ kcount,
                                                       const float* __restrict__ alphas, int n, int H, int W, int max_ctrl, int F, int tiles_x,
                                                       float* out, double* __restrict__ map_out) {
    __shared__ __attribute__((aligned(16))) PwPair pts[PW_MAXK];          // c_k
    __shared__ __attribute__((aligned(16))) PwPair wts[PW_MAXK];          // (w_yk, w_xk)
    __shared__ double aff[6];                                             // a_y0 a_y1 a_y2 a_x0 a_x1 a_x2
    __shared__ uint8_t ids[PG_R * PG_R];
    __shared__ unsigned long long rows[PG_R * PG_T];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * PG_T, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * PG_T;
    const int gy = ty0 + (tid >> 4), gx = tx0 + (tid & 15);
    const bool inside = gy < H && gx < W;
    const size_t HW = (size_t)H * W, plane = (size_t)n * HW, p = (size_t)gy * W + gx;
    const int K = min(max(kcount[b], 0), max_ctrl);          // (a count outside 0 .. max_ctrl never indexes outside the arrays)

    pg_stage_ids(src_masks + (size_t)b * HW, plane, H, W, F, ty0, tx0, tid, ids);
    __syncthreads();
    pg_row_counts(ids, F, tid, rows);
    __syncthreads();
    const unsigned long long cnt = inside ? pg_window_counts(rows, F, tid) : 0ull;
    const bool blend = K > 0 && cnt != 0;
    if (!__syncthreads_or(blend || (map_out != nullptr && K > 0))) {          // nothing to evaluate in this tile: out = xh, q = p
        if (inside) {
            if (out != xh) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[((size_t)b * 3 + c) * HW + p] = xh[((size_t)b * 3 + c) * HW + p];
            }
            if (map_out) {
                map_out[((size_t)b * 2 + 0) * HW + p] = (double)gy;
                map_out[((size_t)b * 2 + 1) * HW + p] = (double)gx;
            }
        }
        return;
    }
    for (int i = tid; i < 2 * K; i += 256) {
        ((double*)pts)[i] = ctrl[(size_t)b * max_ctrl * 2 + i];
        const int d = i & 1, k = i >> 1;
        ((double*)wts)[i] = coef[((size_t)b * 2 + d) * (max_ctrl + 3) + k];
    }
    if (tid < 6) aff[tid] = coef[((size_t)b * 2 + tid / 3) * (max_ctrl + 3) + max_ctrl + tid % 3];
    __syncthreads();
    if (!inside) return;

    double Wt = 0.0, qy = (double)gy, qx = (double)gx;
    double fy = 0.0, fx = 0.0;
    size_t t00 = 0, t01 = 0, t10 = 0, t11 = 0;          // the four taps, indices clamped to the image
    if (blend || map_out) {
        const double py = (double)gy, px = (double)gx;
        double sy = 0.0, sx = 0.0;
        for (int k = 0; k < K; ++k) {
            const PwPair c = pts[k], w = wts[k];
            const double dy = py - c.y, dx = px - c.x;
            const double s = dy * dy + dx * dx;
            const double u = s > 0.0 ? s * log(s) : 0.0;
            sy = sy + w.y * u;
            sx = sx + w.x * u;
        }
        qy = ((sy + aff[0]) + aff[1] * py) + aff[2] * px;
        qx = ((sx + aff[3]) + aff[4] * py) + aff[5] * px;
    }
    if (map_out) {
        map_out[((size_t)b * 2 + 0) * HW + p] = qy;
        map_out[((size_t)b * 2 + 1) * HW + p] = qx;
    }
    if (blend && qy > -1.0 && qy < (double)H && qx > -1.0 && qx < (double)W) {          // (false for a NaN q)
        const double y0f = floor(qy), x0f = floor(qx);
        const int y0 = (int)y0f, x0 = (int)x0f;          // -1 .. H - 1, -1 .. W - 1
        fy = qy - y0f;
        fx = qx - x0f;
        const bool iy0 = y0 >= 0, iy1 = y0 + 1 < H, ix0 = x0 >= 0, ix1 = x0 + 1 < W;
        const size_t r0 = (size_t)max(y0, 0) * W, r1 = (size_t)min(y0 + 1, H - 1) * W;
        const int c0 = max(x0, 0), c1 = min(x0 + 1, W - 1);
        t00 = r0 + c0, t01 = r0 + c1, t10 = r1 + c0, t11 = r1 + c1;
        const double Kw = (double)((2 * F + 1) * (2 * F + 1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = pg_count(cnt, r);
            if (c == 0) continue;          // (its term is +0)
            const double w = pg_weight(alphas[(size_t)b * 4 + pg_mask_plane(r)], c, Kw);
            const uint8_t* m = ref_masks + ((size_t)pg_mask_plane(r) * n + b) * HW;
            const double v00 = iy0 && ix0 && m[t00] ? 1.0 : 0.0, v01 = iy0 && ix1 && m[t01] ? 1.0 : 0.0;
            const double v10 = iy1 && ix0 && m[t10] ? 1.0 : 0.0, v11 = iy1 && ix1 && m[t11] ? 1.0 : 0.0;
            Wt = Wt + w * pw_bilinear(v00, v01, v10, v11, fy, fx);
        }
        Wt = Wt < 1.0 ? Wt : 1.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t e = ((size_t)b * 3 + c) * HW;
        const float x = xh[e + p];
        float o = x;
        if (Wt != 0.0) {
            const float* rc = ref + e;
            const double R = pw_bilinear(pw_colour(rc[t00]), pw_colour(rc[t01]), pw_colour(rc[t10]), pw_colour(rc[t11]), fy, fx);
            o = (float)((double)x + Wt * (R - (double)x));
        }
        if (out != xh || Wt != 0.0) out[e + p] = o;
    }
}

inline bool pw_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

int mkd_pgt_warp_launches(void) { return 1; }

int mkd_pgt_warp(const float* xh, const float* ref, const uint8_t* src_masks, const uint8_t* ref_masks, const double* ctrl, const double* coef,
                 const int32_t* kcount, const float* alphas, int n, int H, int W, int max_ctrl, int feather, float* out, double* map_out,
                 void* stream) {
    const std::string who = "mkd_pgt_warp: ";
    if (!xh || !ref || !src_masks || !ref_masks || !ctrl || !coef || !kcount || !alphas || !out)
        return mkd_fail(MKD_ERR_ARG, who + "null xh / ref / src_masks / ref_masks / ctrl / coef / kcount / alphas / out");
    if (n < 1 || n > 65535 || H < 1 || W < 1 || (int64_t)H * W > (1 << 24))
        return mkd_fail(MKD_ERR_ARG, who + "1 <= n <= 65535 images of [3, H, W] with H * W <= 2^24");
    if (feather < 0 || feather > PG_MAXF) return mkd_fail(MKD_ERR_ARG, who + "feather must be 0..8");
    if (max_ctrl < 1 || max_ctrl > PW_MAXK) return mkd_fail(MKD_ERR_ARG, who + "max_ctrl must be 1..128");
    if (!pw_aligned(xh, 4) || !pw_aligned(ref, 4) || !pw_aligned(out, 4) || !pw_aligned(alphas, 4) || !pw_aligned(kcount, 4))
        return mkd_fail(MKD_ERR_ARG, who + "fp32 and int32 arrays must be 4-byte aligned");
    if (!pw_aligned(ctrl, 8) || !pw_aligned(coef, 8) || !pw_aligned(map_out, 8))
        return mkd_fail(MKD_ERR_ARG, who + "double arrays must be 8-byte aligned");
    const uintptr_t x0 = (uintptr_t)xh, r0 = (uintptr_t)ref, o0 = (uintptr_t)out, bytes = (uintptr_t)n * 3 * (uintptr_t)H * (uintptr_t)W * sizeof(float);
    if (r0 < o0 + bytes && o0 < r0 + bytes) return mkd_fail(MKD_ERR_ARG, who + "out may not overlap ref");
    if (x0 != o0 && x0 < o0 + bytes && o0 < x0 + bytes) return mkd_fail(MKD_ERR_ARG, who + "out must be xh itself or not overlap it");
    const int tiles_x = (W + PG_T - 1) / PG_T, tiles_y = (H + PG_T - 1) / PG_T;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n), block(256);
    hipLaunchKernelGGL(pgt_warp_kernel, grid, block, 0, (hipStream_t)stream, xh, ref, src_masks, ref_masks, ctrl, coef, kcount, alphas, n, H, W,
                       max_ctrl, feather, tiles_x, out, map_out);
    MKD_LAUNCH_CHECK("pgt_warp_kernel");
    return 0;
}
