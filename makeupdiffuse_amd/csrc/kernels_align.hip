// Tilted faces (include/mkd.h: mkd_crop_frame, mkd_paste_frame, mkd_face_frames): the photo path along a rotated square instead of an
// axis-aligned box.  Context-free; the calls only enqueue.  The arithmetic of the crop and the paste is IEEE double with nothing
// contracted (every product that feeds an addition is a mkd_rounded_mul, mkd_common.h), that of the frames
// is 64-bit integer except for one direction per face: tests/photo_frame_ref.py restates all of it operation for operation.
//
// Crop: one launch, a thread owns one output pixel (its three channels and one weight sum) and walks the photo pixels whose tent
// weight in the face's frame can be non-zero, Y outer, X inner.  Paste: one launch over the axis-aligned bounding rectangle of the
// rotated square (one pixel of slack per side, clipped to the photo); a thread owns one photo pixel column of a 64 x 16 tile and tests
// every pixel against the square itself, so the rectangle decides nothing; mkd_paste_frame_guided is the same kernel with the
// four-neighbour interpolation replaced by the guided taps of paste_guided.h, one instantiation per radius.  Frames: four launches -- clear the moments, the eye moments
// (per workgroup in LDS, then one global 64-bit atomic per non-zero cell), one thread per (image, rank) for the direction, the extents
// along that direction (64-bit atomic min / max, again per workgroup first).  No workgroup waits for another.
#include "mkd_common.h"
#include "paste_guided.h"
#include "../../include/mkd.h"

#include <limits.h>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int CF_TW = 16, CF_TH = 16;     // crop tile: one output pixel per thread
constexpr int PF_TW = 64, PF_TH = 16;     // paste tile (kernels_photo.hip's)
constexpr int FF_NT = 256;                // threads of the two per-pixel frame kernels
constexpr int FF_PER = 4;                 // consecutive pixels per thread
constexpr int FF_MAX_OUT = 64;
constexpr int FF_CELLS = 6;               // n_a, sum x, sum y of class set a, then of class set b
constexpr int FF_UNIT = 16384;            // |(cq, sq)|

static_assert(sizeof(mkd_face_frame) == 48, "mkd_face_frame is four int32 and four int64");

struct FrArgs {
    mkd_photo_frame_desc d[MKD_PHOTO_MAX_BATCH];
};
struct PfArgs {
    mkd_photo_frame_desc d[MKD_PHOTO_MAX_BATCH];
    int rx0[MKD_PHOTO_MAX_BATCH], ry0[MKD_PHOTO_MAX_BATCH], rw[MKD_PHOTO_MAX_BATCH], rh[MKD_PHOTO_MAX_BATCH];      // the rectangle the grid covers
};
struct FfArgs {
    int hw[MKD_PHOTO_MAX_BATCH][2];       // H, W of the photo of image b
};

__device__ __forceinline__ int al_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned char al_byte(double o) {
    const double r = rint(o);
    return (unsigned char)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
}

// ---- mkd_crop_frame ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CF_TW * CF_TH) void crop_frame_kernel(const FrArgs a, int S, float* __restrict__ img01, unsigned char* __restrict__ u8_out,
                                                                  unsigned char* __restrict__ labels_out) {
    const int b = blockIdx.z;
    const int j = blockIdx.x * CF_TW + (threadIdx.x % CF_TW), i = blockIdx.y * CF_TH + (threadIdx.x / CF_TW);
    if (i >= S || j >= S) return;
    const mkd_photo_frame_desc d = a.d[b];
    const double scale = d.side / (double)S;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double half = d.side * 0.5;
    const double u = mkd_rounded_mul((double)j + 0.5, scale) - half, v = mkd_rounded_mul((double)i + 0.5, scale) - half;
    const double qx = (d.cx + mkd_rounded_mul(d.c, u)) - mkd_rounded_mul(d.s, v);
    const double qy = (d.cy + mkd_rounded_mul(d.s, u)) + mkd_rounded_mul(d.c, v);
    const double R = mkd_rounded_mul(fs, fabs(d.c) + fabs(d.s));
    // |q| <= 16384 + 33 * 1024 * 2 and R <= 46341: every bound fits an int
    const int xa = (int)floor(qx - R), xb = (int)floor(qx + R);
    const int ya = (int)floor(qy - R), yb = (int)floor(qy + R);
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int Y = ya; Y <= yb; ++Y) {
        const double dy = ((double)Y + 0.5) - qy;
        const double sdy = mkd_rounded_mul(d.s, dy), cdy = mkd_rounded_mul(d.c, dy);
        const unsigned char* row = d.pixels + (size_t)al_clampi(Y, 0, d.H - 1) * d.pitch_bytes;
        for (int X = xa; X <= xb; ++X) {
            const double dx = ((double)X + 0.5) - qx;
            const double du = mkd_rounded_mul(d.c, dx) + sdy;
            const double dv = cdy - mkd_rounded_mul(d.s, dx);
            const double wu = 1.0 - fabs(du) / fs, wv = 1.0 - fabs(dv) / fs;
            if (!(wu > 0.0) || !(wv > 0.0)) continue;          // a zero weight adds +0.0 to every sum: skipping it changes no bit
            const double w = mkd_rounded_mul(wu, wv);
            const unsigned char* p = row + (size_t)al_clampi(X, 0, d.W - 1) * 3;
            sw += w;
            s0 += mkd_rounded_mul(w, (double)p[0]);
            s1 += mkd_rounded_mul(w, (double)p[1]);
            s2 += mkd_rounded_mul(w, (double)p[2]);
        }
    }
    const unsigned char o0 = al_byte(s0 / sw), o1 = al_byte(s1 / sw), o2 = al_byte(s2 / sw);
    const size_t pix = ((size_t)b * S + i) * S + j;
    if (u8_out) {
        u8_out[pix * 3] = o0;
        u8_out[pix * 3 + 1] = o1;
        u8_out[pix * 3 + 2] = o2;
    }
    if (img01) {
        const size_t plane = (size_t)S * S, at = (size_t)b * 3 * plane + (size_t)i * S + j;
        img01[at] = __fdiv_rn((float)o0, 255.0f);
        img01[at + plane] = __fdiv_rn((float)o1, 255.0f);
        img01[at + 2 * plane] = __fdiv_rn((float)o2, 255.0f);
    }
    if (labels_out) {
        const int lx = al_clampi((int)floor(qx), 0, d.W - 1), ly = al_clampi((int)floor(qy), 0, d.H - 1);
        labels_out[pix] = d.labels[(size_t)ly * d.W + lx];
    }
}

// ---- mkd_paste_frame -----------------------------------------------------------------------------------------------------------------
// one axis of the weight plane: mkd_paste_photo_weighted's integers, the quotient in double
__device__ __forceinline__ void pf_plane_axis(int X, int len, int n, int* i0, int* i1, double* w) {
    const int num = (2 * X + 1) * n - len, den = 2 * len;            // |num| < 2^27
    int q = num / den;
    if (num < 0 && q * den != num) --q;                              // floor
    const int rem = num - q * den;
    *w = (double)rem / (double)den;
    *i0 = al_clampi(q, 0, n - 1);
    *i1 = al_clampi(q + 1, 0, n - 1);
}
// one axis of the sample: gu = (u + side / 2) / scale - 0.5, its floor (|gu| <= 32 S + 1; returned, NOT clamped), the clamped
// neighbours and the weight of the upper one
__device__ __forceinline__ int pf_axis(double u, double half, double scale, int S, int* i0, int* i1, double* w) {
    const double g = (u + half) / scale - 0.5;
    const double f = floor(g);
    *w = g - f;
    *i0 = al_clampi((int)f, 0, S - 1);
    *i1 = al_clampi((int)f + 1, 0, S - 1);
    return (int)f;
}
__device__ __forceinline__ double pf_lerp(double p, double q, double w) { return p + mkd_rounded_mul(w, q - p); }
__device__ __forceinline__ double pf_diff(float t, float s) { return mkd_rounded_mul(mkd_rounded_mul((double)t + 1.0, 0.5) - (double)s, 255.0); }

// GR >= 0 (mkd_paste_frame_guided, radius GR): val comes from gp_taps (paste_guided.h) in double under the photo pixel's own luminance,
// inv = 1 / (256 sigma); GR = -1 is the bilinear paste and does not read inv.
template <bool WEIGHTED, int GR>
__global__ __launch_bounds__(256) void paste_frame_kernel(const PfArgs a, int S, const float* __restrict__ t, const float* __restrict__ s01, int rho,
                                                          const float* __restrict__ w, int wh, int ww, double inv) {
    const int b = blockIdx.z;
    const int jx = blockIdx.x * PF_TW + (threadIdx.x & (PF_TW - 1));
    if (jx >= a.rw[b]) return;
    const mkd_photo_frame_desc d = a.d[b];
    const int X = a.rx0[b] + jx;                                     // 0 <= X < W: the rectangle is clipped to the photo
    const double scale = d.side / (double)S, half = d.side * 0.5;
    const double rx = ((double)X + 0.5) - d.cx;
    const double crx = mkd_rounded_mul(d.c, rx), srx = mkd_rounded_mul(d.s, rx);
    const double fr = (double)(rho + 1);
    int gx0 = 0, gx1 = 0;
    double ux = 0.0;
    const float* wb = nullptr;
    if (WEIGHTED) {
        pf_plane_axis(X, d.W, ww, &gx0, &gx1, &ux);
        wb = w + (size_t)b * wh * ww;
    }
    const size_t plane = (size_t)S * S;
    const float* tb = t + (size_t)b * 3 * plane;
    const float* sb = s01 + (size_t)b * 3 * plane;
    unsigned char* px = const_cast<unsigned char*>(d.pixels);
    const int i_end = min(a.rh[b], (int)(blockIdx.y + 1) * PF_TH);
    for (int iy = blockIdx.y * PF_TH + (threadIdx.x >> 6); iy < i_end; iy += 256 / PF_TW) {
        const int Y = a.ry0[b] + iy;
        const double ry = ((double)Y + 0.5) - d.cy;
        const double u = crx + mkd_rounded_mul(d.s, ry), v = mkd_rounded_mul(d.c, ry) - srx;
        if (!(u >= -half && u < half && v >= -half && v < half)) continue;          // outside the square: the byte is not touched
        int c0, c1, r0, r1;
        double wx, wy;
        const int qx = pf_axis(u, half, scale, S, &c0, &c1, &wx);
        const int qy = pf_axis(v, half, scale, S, &r0, &r1, &wy);
        const double e = fmin(fmin(u + half, half - u), fmin(v + half, half - v));
        double al = fmin(e + 0.5, fr) / fr;
        if (WEIGHTED) {
            int gy0, gy1;
            double uy;
            pf_plane_axis(Y, d.H, wh, &gy0, &gy1, &uy);
            const float* q0 = wb + (size_t)gy0 * ww;
            const float* q1 = wb + (size_t)gy1 * ww;
            const double g = pf_lerp(pf_lerp((double)q0[gx0], (double)q0[gx1], ux), pf_lerp((double)q1[gx0], (double)q1[gx1], ux), uy);
            al = mkd_rounded_mul(al, g);
        }
        unsigned char* p = px + (size_t)Y * d.pitch_bytes + (size_t)X * 3;
        double val[3];
        if constexpr (GR >= 0) {
            gp_taps<double, GR>(tb, sb, S, qx, wx, qy, wy, (double)gp_luma(p[0], p[1], p[2]), inv, val);    // (the bytes are read before the writes below)
        } else {
            const int o00 = r0 * S + c0, o01 = r0 * S + c1, o10 = r1 * S + c0, o11 = r1 * S + c1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* tc = tb + c * plane;
                const float* sc = sb + c * plane;
                const double d00 = pf_diff(tc[o00], sc[o00]), d01 = pf_diff(tc[o01], sc[o01]);
                const double d10 = pf_diff(tc[o10], sc[o10]), d11 = pf_diff(tc[o11], sc[o11]);
                const double top = pf_lerp(d00, d01, wx), bot = pf_lerp(d10, d11, wx);
                val[c] = pf_lerp(top, bot, wy);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = al_byte((double)p[c] + mkd_rounded_mul(al, val[c]));
    }
}

static_assert(MKD_PHOTO_MAX_BATCH == 16, "mkd_check_photo_descs (mkd_common.h) states the limit and its text as 16");
const char* frame_check(const mkd_photo_frame_desc* descs, int n, int S, bool need_labels) {
    return mkd_check_photo_descs(descs, n, S, need_labels, [S](const mkd_photo_frame_desc& d) -> const char* {
        if (!std::isfinite(d.cx) || !std::isfinite(d.cy) || !std::isfinite(d.side) || !std::isfinite(d.c) || !std::isfinite(d.s))
            return "cx, cy, side, c, s must be finite";
        if (!(d.side > 0.0) || d.side > 32.0 * S) return "side must lie in (0, 32 S]";
        if (!(fabs(d.c * d.c + d.s * d.s - 1.0) <= 1e-9)) return "(c, s) must be a unit vector (|c^2 + s^2 - 1| <= 1e-9)";
        if (d.cx < -d.side || d.cx > (double)d.W + d.side || d.cy < -d.side || d.cy > (double)d.H + d.side)
            return "the centre must lie within side of the photo rectangle";
        return nullptr;
    });
}

template <int GR>
void launch_paste_frame(const dim3 grid, hipStream_t stream, const PfArgs& a, int S, const float* t, const float* s01, int feather,
                        const float* w, int wh, int ww, double inv) {
    if (w)
        hipLaunchKernelGGL((paste_frame_kernel<true, GR>), grid, dim3(256), 0, stream, a, S, t, s01, feather, w, wh, ww, inv);
    else
        hipLaunchKernelGGL((paste_frame_kernel<false, GR>), grid, dim3(256), 0, stream, a, S, t, s01, feather, w, wh, ww, inv);
}

// the one launcher of both paste entries: radius < 0 is the bilinear paste (sigma is not read)
int paste_frame(const std::string who, const mkd_photo_frame_desc* descs, int n, int S, const float* t, const float* s01, int feather,
                const float* w, int wh, int ww, int radius, float sigma, void* stream) {
    if (const char* e = frame_check(descs, n, S, false)) return mkd_fail(MKD_ERR_ARG, who + e);
    if (!t || !s01) return mkd_fail(MKD_ERR_ARG, who + "null t / s01");
    if (feather < 0 || feather > MKD_PHOTO_MAX_FEATHER) return mkd_fail(MKD_ERR_ARG, who + "feather must be 0..64 photo pixels");
    if (w && (wh < 1 || ww < 1 || wh > 2048 || ww > 2048)) return mkd_fail(MKD_ERR_ARG, who + "wh, ww must be 1..2048");
    if (radius >= 0)
        if (const char* e = gp_check(radius, sigma)) return mkd_fail(MKD_ERR_ARG, who + e);
    const double inv = radius >= 0 ? 1.0 / (256.0 * (double)sigma) : 0.0;
    PfArgs a = {};
    int mw = 0, mh = 0;
    for (int i = 0; i < n; ++i) {
        const mkd_photo_frame_desc& d = descs[i];
        a.d[i] = d;
        // the square's corners lie within reach of its centre per axis; one pixel of slack, the kernel tests every pixel itself
        const double reach = d.side * 0.5 * (fabs(d.c) + fabs(d.s));
        const double x_lo = floor(d.cx - reach) - 1.0, x_hi = floor(d.cx + reach) + 1.0;
        const double y_lo = floor(d.cy - reach) - 1.0, y_hi = floor(d.cy + reach) + 1.0;
        const int x0 = (int)(x_lo < 0.0 ? 0.0 : x_lo), x1 = (int)(x_hi > (double)(d.W - 1) ? (double)(d.W - 1) : x_hi);
        const int y0 = (int)(y_lo < 0.0 ? 0.0 : y_lo), y1 = (int)(y_hi > (double)(d.H - 1) ? (double)(d.H - 1) : y_hi);
        a.rx0[i] = x0;
        a.ry0[i] = y0;
        a.rw[i] = x1 >= x0 && y1 >= y0 ? x1 - x0 + 1 : 0;           // 0: the square does not reach the photo
        a.rh[i] = x1 >= x0 && y1 >= y0 ? y1 - y0 + 1 : 0;
        mw = a.rw[i] > mw ? a.rw[i] : mw;
        mh = a.rh[i] > mh ? a.rh[i] : mh;
    }
    if (mw == 0 || mh == 0) return 0;                               // nothing to write
    const dim3 grid((unsigned)((mw + PF_TW - 1) / PF_TW), (unsigned)((mh + PF_TH - 1) / PF_TH), (unsigned)n);      // y <= 1024
    switch (radius) {
        case 0: launch_paste_frame<0>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv); break;
        case 1: launch_paste_frame<1>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv); break;
        case 2: launch_paste_frame<2>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv); break;
        default: launch_paste_frame<-1>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv);
    }
    MKD_LAUNCH_CHECK("paste_frame_kernel");
    return 0;
}


// ---- mkd_face_frames -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ff_in(uint8_t l, uint64_t classes) { return l < 64 && ((classes >> l) & 1ull); }

// the table ids of image b into LDS (wave 0) -> 1 + the last row that holds an id.  Callers put a barrier behind it.
__device__ __forceinline__ void ff_load_ids(const mkd_component* table, int b, int max_out, int* s_id, int* s_rows) {
    if (threadIdx.x < FF_MAX_OUT) {
        const int id = (int)threadIdx.x < max_out ? table[(size_t)b * max_out + threadIdx.x].id : -1;
        s_id[threadIdx.x] = id;
        const unsigned long long held = __ballot(id >= 0);
        if (threadIdx.x == 0) *s_rows = held ? 64 - __clzll((long long)held) : 0;
    }
}
__device__ __forceinline__ int ff_rank(const int* s_id, int rows, int id) {
    for (int r = 0; r < rows; ++r)
        if (s_id[r] == id) return r;                                 // the lowest row of a repeated id
    return -1;
}

__global__ __launch_bounds__(FF_NT) void ff_clear_kernel(unsigned long long* __restrict__ cells, int n) {
    const int k = blockIdx.x * FF_NT + threadIdx.x;
    if (k < n) cells[k] = 0ull;
}

__global__ __launch_bounds__(FF_NT) void ff_moments_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ ids,
                                                           const mkd_component* __restrict__ table, int S, int max_out, uint64_t classes_a,
                                                           uint64_t classes_b, unsigned long long* __restrict__ cells) {
    __shared__ int s_id[FF_MAX_OUT];
    __shared__ int s_rows;
    __shared__ unsigned long long s_cell[FF_MAX_OUT * FF_CELLS];
    const int b = blockIdx.y;
    ff_load_ids(table, b, max_out, s_id, &s_rows);
    for (int k = threadIdx.x; k < FF_MAX_OUT * FF_CELLS; k += FF_NT) s_cell[k] = 0ull;
    __syncthreads();
    const int rows = s_rows;
    const size_t npix = (size_t)S * S, base = (size_t)b * npix;
    const size_t p0 = ((size_t)blockIdx.x * FF_NT + threadIdx.x) * FF_PER;
    int last_id = -1, last_rank = -1;
    for (int k = 0; k < FF_PER; ++k) {
        const size_t p = p0 + k;
        if (p >= npix) break;
        const int id = ids[base + p];
        if (id < 0) continue;
        const uint8_t l = labels[base + p];
        const bool ina = ff_in(l, classes_a), inb = ff_in(l, classes_b);
        if (!ina && !inb) continue;
        if (id != last_id) {
            last_id = id;
            last_rank = ff_rank(s_id, rows, id);
        }
        if (last_rank < 0) continue;
        const unsigned long long x = (unsigned long long)(p % S), y = (unsigned long long)(p / S);
        unsigned long long* c = s_cell + last_rank * FF_CELLS;
        if (ina) {
            atomicAdd(c, 1ull);
            atomicAdd(c + 1, x);
            atomicAdd(c + 2, y);
        }
        if (inb) {
            atomicAdd(c + 3, 1ull);
            atomicAdd(c + 4, x);
            atomicAdd(c + 5, y);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < rows * FF_CELLS; k += FF_NT)
        if (s_cell[k]) atomicAdd(cells + (size_t)b * max_out * FF_CELLS + k, s_cell[k]);
}

// one thread per (image, rank): the direction from the moments, and the frame's extents set to "none yet"
__global__ __launch_bounds__(FF_NT) void ff_direction_kernel(const mkd_component* __restrict__ table, const FfArgs a, int batch, int S, int max_out,
                                                             int min_eye_area, const unsigned long long* __restrict__ cells,
                                                             mkd_face_frame* __restrict__ frames) {
    const int k = blockIdx.x * FF_NT + threadIdx.x;
    if (k >= batch * max_out) return;
    const int b = k / max_out;
    mkd_face_frame f;
    f.n_a = f.n_b = 0;
    f.cq = FF_UNIT;
    f.sq = 0;
    f.umin = f.vmin = INT64_MAX;
    f.umax = f.vmax = INT64_MIN;
    if (table[k].id >= 0) {
        const unsigned long long* c = cells + (size_t)k * FF_CELLS;
        const long long na = (long long)c[0], nb = (long long)c[3];
        f.n_a = (int32_t)na;
        f.n_b = (int32_t)nb;
        if (na >= min_eye_area && nb >= min_eye_area) {
            const double H = (double)a.hw[b][0], W = (double)a.hw[b][1];
            double px = ((double)c[4] / (double)nb - (double)c[1] / (double)na) * (W / (double)S);
            double py = ((double)c[5] / (double)nb - (double)c[2] / (double)na) * (H / (double)S);
            if (px < 0.0) {
                px = -px;
                py = -py;
            }
            const double len = sqrt(mkd_rounded_mul(px, px) + mkd_rounded_mul(py, py));
            if (len != 0.0) {
                const int cq = (int)rint(px / len * 16384.0), sq = (int)rint(py / len * 16384.0);
                if (cq >= FF_UNIT / 2) {
                    f.cq = cq;
                    f.sq = sq;
                }
            }
        }
    }
    frames[k] = f;
}

__global__ __launch_bounds__(FF_NT) void ff_extent_kernel(const int32_t* __restrict__ ids, const mkd_component* __restrict__ table, const FfArgs a, int S,
                                                          int max_out, mkd_face_frame* __restrict__ frames) {
    __shared__ int s_id[FF_MAX_OUT];
    __shared__ int s_rows;
    __shared__ int s_cq[FF_MAX_OUT], s_sq[FF_MAX_OUT];
    __shared__ long long s_lo[FF_MAX_OUT][2], s_hi[FF_MAX_OUT][2];          // [rank][u, v]
    const int b = blockIdx.y;
    ff_load_ids(table, b, max_out, s_id, &s_rows);
    if (threadIdx.x < FF_MAX_OUT) {
        const bool held = (int)threadIdx.x < max_out;
        s_cq[threadIdx.x] = held ? frames[(size_t)b * max_out + threadIdx.x].cq : FF_UNIT;
        s_sq[threadIdx.x] = held ? frames[(size_t)b * max_out + threadIdx.x].sq : 0;
        s_lo[threadIdx.x][0] = s_lo[threadIdx.x][1] = INT64_MAX;
        s_hi[threadIdx.x][0] = s_hi[threadIdx.x][1] = INT64_MIN;
    }
    __syncthreads();
    const int rows = s_rows;
    const long long H = a.hw[b][0], W = a.hw[b][1];
    const size_t npix = (size_t)S * S, base = (size_t)b * npix;
    const size_t p0 = ((size_t)blockIdx.x * FF_NT + threadIdx.x) * FF_PER;
    // a thread's run of pixels of one rank is reduced in registers and goes to LDS once
    int run = -1, last_id = -1, last_rank = -1;
    long long ulo = INT64_MAX, uhi = INT64_MIN, vlo = INT64_MAX, vhi = INT64_MIN;
    auto flush = [&]() {
        if (run < 0) return;
        atomicMin(&s_lo[run][0], ulo);
        atomicMax(&s_hi[run][0], uhi);
        atomicMin(&s_lo[run][1], vlo);
        atomicMax(&s_hi[run][1], vhi);
    };
    for (int k = 0; k < FF_PER; ++k) {
        const size_t p = p0 + k;
        if (p >= npix) break;
        const int id = ids[base + p];
        if (id < 0) continue;
        if (id != last_id) {
            last_id = id;
            last_rank = ff_rank(s_id, rows, id);
        }
        if (last_rank < 0) continue;
        if (last_rank != run) {
            flush();
            run = last_rank;
            ulo = vlo = INT64_MAX;
            uhi = vhi = INT64_MIN;
        }
        const long long X2 = (2 * (long long)(p % S) + 1) * W, Y2 = (2 * (long long)(p / S) + 1) * H;
        const long long cq = s_cq[run], sq = s_sq[run];
        const long long pu = cq * X2 + sq * Y2, pv = -sq * X2 + cq * Y2;          // |.| < 2^43
        ulo = pu < ulo ? pu : ulo;
        uhi = pu > uhi ? pu : uhi;
        vlo = pv < vlo ? pv : vlo;
        vhi = pv > vhi ? pv : vhi;
    }
    flush();
    __syncthreads();
    if ((int)threadIdx.x < rows && s_lo[threadIdx.x][0] != INT64_MAX) {          // a rank with a pixel in this workgroup has all four
        mkd_face_frame* f = frames + (size_t)b * max_out + threadIdx.x;
        atomicMin((long long*)&f->umin, s_lo[threadIdx.x][0]);
        atomicMax((long long*)&f->umax, s_hi[threadIdx.x][0]);
        atomicMin((long long*)&f->vmin, s_lo[threadIdx.x][1]);
        atomicMax((long long*)&f->vmax, s_hi[threadIdx.x][1]);
    }
}

const char* ff_check(int batch, int max_out) {
    if (batch < 1 || batch > MKD_PHOTO_MAX_BATCH) return "batch must be 1..16";
    if (max_out < 1 || max_out > FF_MAX_OUT) return "max_out must be 1..64";
    return nullptr;
}
size_t ff_scratch(int batch, int max_out) { return ((size_t)batch * max_out * FF_CELLS * sizeof(unsigned long long) + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int mkd_crop_frame(const mkd_photo_frame_desc* descs, int n, int S, float* img01, uint8_t* u8_out, uint8_t* labels_out, void* stream) {
    const std::string who = "mkd_crop_frame: ";
    if (const char* e = frame_check(descs, n, S, labels_out != nullptr)) return mkd_fail(MKD_ERR_ARG, who + e);
    if (!img01 && !u8_out) return mkd_fail(MKD_ERR_ARG, who + "img01 and u8_out are both null");
    FrArgs a = {};
    for (int i = 0; i < n; ++i) a.d[i] = descs[i];
    const dim3 grid((unsigned)((S + CF_TW - 1) / CF_TW), (unsigned)((S + CF_TH - 1) / CF_TH), (unsigned)n);
    hipLaunchKernelGGL(crop_frame_kernel, grid, dim3(CF_TW * CF_TH), 0, (hipStream_t)stream, a, S, img01, u8_out, labels_out);
    MKD_LAUNCH_CHECK("crop_frame_kernel");
    return 0;
}

int mkd_paste_frame(const mkd_photo_frame_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w, int wh,
                    int ww, void* stream) {
    return paste_frame("mkd_paste_frame: ", descs, n, S, t, s01, feather, w, wh, ww, -1, 0.0f, stream);
}

int mkd_paste_frame_guided(const mkd_photo_frame_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w,
                           int wh, int ww, int radius, float sigma, void* stream) {
    if (radius < 0) return mkd_fail(MKD_ERR_ARG, std::string("mkd_paste_frame_guided: ") + gp_check(radius, sigma));
    return paste_frame("mkd_paste_frame_guided: ", descs, n, S, t, s01, feather, w, wh, ww, radius, sigma, stream);
}

size_t mkd_face_frames_scratch_bytes(int batch, int max_out) {
    if (const char* e = ff_check(batch, max_out)) {
        mkd_set_error(std::string("mkd_face_frames_scratch_bytes: ") + e);
        return 0;
    }
    return ff_scratch(batch, max_out);
}

int mkd_face_frames(const uint8_t* labels, const int32_t* ids, const mkd_component* table, int batch, int S, int max_out, const int32_t* photo_hw,
                    uint64_t classes_a, uint64_t classes_b, int min_eye_area, mkd_face_frame* frames, void* scratch, void* stream) {
    const std::string who = "mkd_face_frames: ";
    if (const char* e = ff_check(batch, max_out)) return mkd_fail(MKD_ERR_ARG, who + e);
    if (S < 1 || S > 4096) return mkd_fail(MKD_ERR_ARG, who + "S must be 1..4096");
    if (min_eye_area < 1) return mkd_fail(MKD_ERR_ARG, who + "min_eye_area must be >= 1");
    if (!labels || !ids || !table || !photo_hw || !frames) return mkd_fail(MKD_ERR_ARG, who + "null labels / ids / table / photo_hw / frames");
    if (!scratch || ((uintptr_t)scratch & 255)) return mkd_fail(MKD_ERR_ARG, who + "the scratch must be a 256-byte aligned device buffer");
    FfArgs a = {};
    for (int b = 0; b < batch; ++b) {
        a.hw[b][0] = photo_hw[2 * b];
        a.hw[b][1] = photo_hw[2 * b + 1];
        if (a.hw[b][0] < 1 || a.hw[b][0] > 16384 || a.hw[b][1] < 1 || a.hw[b][1] > 16384)
            return mkd_fail(MKD_ERR_ARG, who + "photo H, W must be 1..16384");
    }
    const hipStream_t st = (hipStream_t)stream;
    unsigned long long* cells = (unsigned long long*)scratch;
    const int ncells = batch * max_out * FF_CELLS, nrows = batch * max_out;
    const dim3 pix((unsigned)(((size_t)S * S + (size_t)FF_NT * FF_PER - 1) / ((size_t)FF_NT * FF_PER)), (unsigned)batch);      // x <= 16384
    hipLaunchKernelGGL(ff_clear_kernel, dim3((unsigned)((ncells + FF_NT - 1) / FF_NT)), dim3(FF_NT), 0, st, cells, ncells);
    MKD_LAUNCH_CHECK("ff_clear_kernel");
    hipLaunchKernelGGL(ff_moments_kernel, pix, dim3(FF_NT), 0, st, labels, ids, table, S, max_out, classes_a, classes_b, cells);
    MKD_LAUNCH_CHECK("ff_moments_kernel");
    hipLaunchKernelGGL(ff_direction_kernel, dim3((unsigned)((nrows + FF_NT - 1) / FF_NT)), dim3(FF_NT), 0, st, table, a, batch, S, max_out,
                       min_eye_area, (const unsigned long long*)cells, frames);
    MKD_LAUNCH_CHECK("ff_direction_kernel");
    hipLaunchKernelGGL(ff_extent_kernel, pix, dim3(FF_NT), 0, st, ids, table, a, S, max_out, frames);
    MKD_LAUNCH_CHECK("ff_extent_kernel");
    return 0;
}

}  // extern "C"
