// Guided paste (include/mkd.h: mkd_paste_photo_guided, mkd_paste_frame_guided): the tap loop both paste kernels share.  The makeup
// difference d of the (2 R + 2)^2 model pixels around a photo pixel is averaged with tent weights in model pixels times a Cauchy weight
// on the luminance distance between the photo pixel and the model pixel (joint bilateral upsampling, Kopf et al. 2007), so the
// difference stops at the photo's own edges.  T is float for the box kernel and double for the frame kernel; d and the low-resolution
// luminance are fp32 in both and widened.  Every operator is one correctly rounded operation: products that feed an addition pass
// through mkd_rounded.  Each tap reads t and s01 straight from the L2-resident tensors.
#pragma once
#include "mkd_common.h"

// d = ((t + 1) 0.5 - s01) 255 of one model pixel and channel, fp32
__device__ __forceinline__ float pp_diff(float t, float s) {
    const float r = mkd_rounded(__fmul_rn(__fadd_rn(t, 1.0f), 0.5f));
    return mkd_rounded(__fmul_rn(__fsub_rn(r, s), 255.0f));
}

__device__ __forceinline__ float gp_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double gp_div(double a, double b) { return a / b; }
__device__ __forceinline__ int gp_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// 77 R + 150 G + 29 B: 256 times the luminance in 8-bit levels, an integer <= 65280
__device__ __forceinline__ int gp_luma(int r, int g, int b) { return 77 * r + 150 * g + 29 * b; }
__device__ __forceinline__ int gp_byte(float s) { return (int)fminf(fmaxf(rintf(__fmul_rn(s, 255.0f)), 0.0f), 255.0f); }

// tent weight of tap m (-R .. R + 1) of one axis: 1 - dist / (R + 1) with dist the distance in model pixels from the sample point,
// which lies w in [0, 1) beyond tap 0
template <typename T>
__device__ __forceinline__ T gp_tent(int m, T w, T invT) {
    const T dist = m >= 1 ? (T)m - w : w + (T)(-m);
    return (T)1 - mkd_rounded(dist * invT);
}

// u[c] = sum g d_c / sum g over the taps (my outer, mx inner, both ascending) around the unclamped model pixel (qy, qx) with the
// fractions (wy, wx); tb / sb = t / s01 of this image, yh = float(77 R + 150 G + 29 B) of the photo pixel, inv = 1 / (256 sigma)
template <typename T, int R>
__device__ __forceinline__ void gp_taps(const float* __restrict__ tb, const float* __restrict__ sb, int S, int qx, T wx, int qy, T wy, T yh,
                                        T inv, T* u) {
#pragma clang fp contract(off)
    const size_t plane = (size_t)S * S;
    const T invT = gp_div((T)1, (T)(R + 1));
    T wsx[2 * R + 2];
    int ox[2 * R + 2];
#pragma unroll
    for (int mx = -R; mx <= R + 1; ++mx) {
        wsx[mx + R] = gp_tent(mx, wx, invT);
        ox[mx + R] = gp_clampi(qx + mx, 0, S - 1);
    }
    T sw = (T)0, sc0 = (T)0, sc1 = (T)0, sc2 = (T)0;
    for (int my = -R; my <= R + 1; ++my) {
        const T wsy = gp_tent(my, wy, invT);
        const int row = gp_clampi(qy + my, 0, S - 1) * S;
#pragma unroll
        for (int k = 0; k < 2 * R + 2; ++k) {
            const int o = row + ox[k];
            const float s0 = sb[o], s1 = sb[plane + o], s2 = sb[2 * plane + o];
            const float d0 = pp_diff(tb[o], s0), d1 = pp_diff(tb[plane + o], s1), d2 = pp_diff(tb[2 * plane + o], s2);
            const T yl = (T)(float)gp_luma(gp_byte(s0), gp_byte(s1), gp_byte(s2));
            const T q = mkd_rounded((yh - yl) * inv);
            const T wr = gp_div((T)1, (T)1 + mkd_rounded(q * q));
            const T g = mkd_rounded(mkd_rounded(wsy * wsx[k]) * wr);
            sw = sw + g;
            sc0 = sc0 + mkd_rounded(g * (T)d0);
            sc1 = sc1 + mkd_rounded(g * (T)d1);
            sc2 = sc2 + mkd_rounded(g * (T)d2);
        }
    }
    u[0] = gp_div(sc0, sw);
    u[1] = gp_div(sc1, sw);
    u[2] = gp_div(sc2, sw);
}

// radius, sigma of a guided entry: the text of the first rule broken, else null
inline const char* gp_check(int radius, float sigma) {
    if (radius < 0 || radius > 2) return "radius must be 0, 1 or 2";
    if (!(sigma >= 0.5f && sigma <= 1e6f)) return "sigma must be finite, 0.5 .. 1e6 luminance levels";
    return nullptr;
}
