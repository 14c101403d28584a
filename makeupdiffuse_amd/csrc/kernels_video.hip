// Video clips (include/mkd.h: mkd_temporal_diff): a motion-aware recursive filter over time of the makeup difference
// d = (t + 1) / 2 - s01 that the paste kernels add to the photo.  d lives at model resolution in the face's own frame (the crop follows
// the face), so pixel p of frame k and pixel p of frame k - 1 show the same place of the face and a per-pixel filter is meaningful.
// The confidence of the previous frame's value is a Cauchy weight on the mean absolute luminance change of the (2 R + 1)^2 window
// around the pixel, so a cut, a hand in front of the face or a blink restart the filter where they happen and nowhere else.  The
// filtered difference goes back into t (t_out = (s01 + D) 2 - 1): every paste kernel then sees it, unchanged.
//
// One thread per model pixel, 16 x 16 per workgroup, the three channels in the same thread.  The luminance of the tile plus its halo,
// of this frame (formed from s01) and of the previous one (the Y pool), is staged in LDS as integers: each would otherwise be read
// (2 R + 1)^2 times per pixel.  The staging loop and the barrier are uniform over the workgroup: a face without a previous frame stages
// zeros and takes its branch after the barrier, on data.  fp32, one correctly rounded operation per operator (mkd_rounded keeps
// products out of fused multiply-adds); the window sum is a sum of integers.
#include "mkd_common.h"
#include "paste_guided.h"
#include "../../include/mkd.h"

namespace {

constexpr int TD_T = 16;          // tile side: TD_T x TD_T threads

struct TdArgs {
    int32_t slot_in[MKD_PHOTO_MAX_BATCH];
    int32_t slot_out[MKD_PHOTO_MAX_BATCH];
};

template <int R>
__global__ __launch_bounds__(TD_T * TD_T) void temporal_diff_kernel(const TdArgs a, int S, const float* t,          // (t_out may be t)
                                                                     const float* __restrict__ s01, const float* __restrict__ D_in,
                                                                     const float* __restrict__ Y_in, float* __restrict__ D_out,
                                                                     float* __restrict__ Y_out, float beta, float inv, float* t_out) {
    constexpr int HW = TD_T + 2 * R;          // tile plus halo
    __shared__ int y_cur[HW * HW];
    __shared__ int y_old[HW * HW];
    const int b = blockIdx.z;
    const int si = a.slot_in[b], so = a.slot_out[b];
    const bool first = si < 0;
    const size_t plane = (size_t)S * S;
    const float* sb = s01 + (size_t)b * 3 * plane;
    const float* yi = first ? nullptr : Y_in + (size_t)si * plane;
    const int ty0 = blockIdx.y * TD_T, tx0 = blockIdx.x * TD_T;
    // every thread runs the same number of rounds (HW * HW and the block size are constants) and reaches the barrier
    for (int e = threadIdx.x; e < HW * HW; e += TD_T * TD_T) {
        const int gy = gp_clampi(ty0 + e / HW - R, 0, S - 1), gx = gp_clampi(tx0 + e % HW - R, 0, S - 1);
        const size_t o = (size_t)gy * S + gx;
        y_cur[e] = gp_luma(gp_byte(sb[o]), gp_byte(sb[plane + o]), gp_byte(sb[2 * plane + o]));
        y_old[e] = first ? 0 : (int)yi[o];
    }
    __syncthreads();
    const int lx = threadIdx.x % TD_T, ly = threadIdx.x / TD_T;
    const int x = tx0 + lx, y = ty0 + ly;
    if (x >= S || y >= S) return;          // (after the only barrier)
    const size_t o = (size_t)y * S + x;
    const float* tb = t + (size_t)b * 3 * plane;
    float* ob = t_out + (size_t)b * 3 * plane;
    float* dout = D_out + (size_t)so * 3 * plane;
    Y_out[(size_t)so * plane + o] = (float)y_cur[(ly + R) * HW + lx + R];
    float k = 0.0f;
    const float* din = nullptr;
    if (!first) {
        int A = 0;
#pragma unroll
        for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2 * R; ++dx) {
                const int e = (ly + dy) * HW + lx + dx;
                A += abs(y_cur[e] - y_old[e]);
            }
        const float q = __fmul_rn((float)A, inv);
        const float c = __fdiv_rn(1.0f, __fadd_rn(1.0f, mkd_rounded(__fmul_rn(q, q))));
        k = __fmul_rn(beta, c);
        din = D_in + (size_t)si * 3 * plane;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t oc = c * plane + o;
        const float tv = tb[oc], sv = sb[oc];
        const float d = __fsub_rn(mkd_rounded(__fmul_rn(__fadd_rn(tv, 1.0f), 0.5f)), sv);
        if (first) {
            dout[oc] = d;
            ob[oc] = tv;
        } else {
            const float D = __fadd_rn(d, mkd_rounded(__fmul_rn(k, __fsub_rn(din[oc], d))));
            dout[oc] = D;
            ob[oc] = __fsub_rn(mkd_rounded(__fmul_rn(__fadd_rn(sv, D), 2.0f)), 1.0f);
        }
    }
}

bool td_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

template <int R>
void launch_td(const dim3 grid, hipStream_t stream, const TdArgs& a, int S, const float* t, const float* s01, const float* D_in,
               const float* Y_in, float* D_out, float* Y_out, float beta, float inv, float* t_out) {
    hipLaunchKernelGGL((temporal_diff_kernel<R>), grid, dim3(TD_T * TD_T), 0, stream, a, S, t, s01, D_in, Y_in, D_out, Y_out, beta, inv, t_out);
}

}  // namespace

extern "C" {

int mkd_temporal_diff(const float* t, const float* s01, int n, int S, const float* D_in, const float* Y_in, const int32_t* slot_in,
                      float* D_out, float* Y_out, const int32_t* slot_out, int pool, float beta, float tau, int radius, float* t_out,
                      void* stream) {
    const std::string who = "mkd_temporal_diff: ";
    if (!t || !s01 || !D_in || !Y_in || !slot_in || !D_out || !Y_out || !slot_out || !t_out) return mkd_fail(MKD_ERR_ARG, who + "null pointer");
    if (n < 1 || n > MKD_PHOTO_MAX_BATCH) return mkd_fail(MKD_ERR_ARG, who + "1..16 faces per call");
    if (S < 8 || S > 1024) return mkd_fail(MKD_ERR_ARG, who + "S must be 8..1024");
    if (radius < 0 || radius > 2) return mkd_fail(MKD_ERR_ARG, who + "radius must be 0, 1 or 2");
    if (!(beta > 0.0f && beta <= 0.95f)) return mkd_fail(MKD_ERR_ARG, who + "beta must lie in (0, 0.95]");
    if (!(tau >= 0.5f && tau <= 1e6f)) return mkd_fail(MKD_ERR_ARG, who + "tau must be finite, 0.5 .. 1e6 luminance levels");
    if (pool < 1 || pool > 65536) return mkd_fail(MKD_ERR_ARG, who + "pool must hold 1..65536 slots");
    TdArgs a = {};
    for (int i = 0; i < n; ++i) {
        if (slot_in[i] < -1 || slot_in[i] >= pool) return mkd_fail(MKD_ERR_ARG, who + "slot_in must be -1 or a slot of the pool");
        if (slot_out[i] < 0 || slot_out[i] >= pool) return mkd_fail(MKD_ERR_ARG, who + "slot_out must be a slot of the pool");
        for (int j = 0; j < i; ++j)
            if (slot_out[j] == slot_out[i]) return mkd_fail(MKD_ERR_ARG, who + "slot_out must not repeat");
        a.slot_in[i] = slot_in[i];
        a.slot_out[i] = slot_out[i];
    }
    const size_t yb = (size_t)pool * S * S * sizeof(float), db = 3 * yb;
    if (td_overlap(D_in, db, D_out, db) || td_overlap(D_in, db, Y_out, yb) || td_overlap(Y_in, yb, D_out, db) || td_overlap(Y_in, yb, Y_out, yb) ||
        td_overlap(D_out, db, Y_out, yb))
        return mkd_fail(MKD_ERR_ARG, who + "the _in pools, D_out and Y_out must not overlap");
    const int taps = (2 * radius + 1) * (2 * radius + 1);
    volatile float scale = 256.0f * tau;          // (volatile: each product is rounded to fp32 on its own)
    volatile float den = scale * (float)taps;
    const float inv = 1.0f / den;
    const unsigned tiles = (unsigned)((S + TD_T - 1) / TD_T);
    const dim3 grid(tiles, tiles, (unsigned)n);
    switch (radius) {
        case 0: launch_td<0>(grid, (hipStream_t)stream, a, S, t, s01, D_in, Y_in, D_out, Y_out, beta, inv, t_out); break;
        case 1: launch_td<1>(grid, (hipStream_t)stream, a, S, t, s01, D_in, Y_in, D_out, Y_out, beta, inv, t_out); break;
        default: launch_td<2>(grid, (hipStream_t)stream, a, S, t, s01, D_in, Y_in, D_out, Y_out, beta, inv, t_out);
    }
    MKD_LAUNCH_CHECK("temporal_diff_kernel");
    return 0;
}

}  // extern "C"
