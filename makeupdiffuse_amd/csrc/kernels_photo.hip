// Full-resolution photos (include/mkd.h: mkd_crop_resize, mkd_resize_coeffs, mkd_paste_photo): any-size uint8 photo + box -> the
// model's S x S input with the bytes of Pillow's antialiased bilinear resize, and the decoded sample back into the photo at its own
// resolution.  Context-free; the calls only enqueue.
//
// Crop-resize: Pillow's two-pass integer resampler (Resample.c: precompute_coeffs / normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc
// / ImagingResampleVertical_8bpc), restated.  rs_axis_coeffs builds one output index's bounds and 2^22 fixed-point coefficients in fp64
// with nothing contracted; a block builds the table of its RS_G output columns (horizontal) or rows (vertical) into LDS, one lane per
// index, and then all 256 threads filter.  Launch 1, horizontal: photo rows [rbase, rbase + rows) (the rows the vertical filter
// reads: it reaches its support beyond the box, rs_rows) -> scratch uint8 [rows][S][3]; grid (ceil(S / 32), ceil(max rows / 64), n),
// a thread owns one (row, column) and its three channels.  Launch 2, vertical: scratch -> img01 / u8_out / labels_out; grid
// (ceil(3 S / 256), ceil(S / 8), n), a thread owns one interleaved byte column of 8 output rows (coalesced scratch reads).
//
// Paste: one launch, a thread owns one photo pixel column of a 64 x 16 box tile (4 rows); the model-resolution difference
// d = ((t + 1) 0.5 - s01) 255 is formed on the fly from the L2-resident tensors.  Every fp32 operation is one correctly rounded step:
// products that feed an addition pass through mkd_rounded (mkd_common.h).
// mkd_paste_photo_weighted is the same kernel's second instantiation: the feather weight times a bilinear sample of a photo-wide plane.
// mkd_paste_photo_guided is the same kernel with the four-neighbour interpolation replaced by the guided taps of paste_guided.h, one
// instantiation per radius.
#include "mkd_common.h"
#include "paste_guided.h"
#include "../../include/mkd.h"

namespace {

constexpr int RS_G = 32;              // output columns per block of the horizontal pass
constexpr int RS_GV = 8;              // output rows per block of the vertical pass
constexpr int RS_KMAX = 67;           // 2 ceil(support) + 1 with support <= 32 is 65; odd, so LDS rows of the table do not share banks
constexpr int RS_ROWS = 64;           // photo rows per block of the horizontal pass
constexpr int PP_TW = 64, PP_TH = 16; // paste tile

struct RsArgs {
    mkd_photo_desc d[MKD_PHOTO_MAX_BATCH];
    unsigned long long off[MKD_PHOTO_MAX_BATCH];          // byte offset of a photo's slab in the scratch
};
struct PpArgs {
    mkd_photo_desc d[MKD_PHOTO_MAX_BATCH];
};

// ceil(max(len / S, 1)) = ceil(support): a non-integer len / S is at least 1 / 1024 away from an integer, so the double agrees
__host__ __device__ inline int rs_csupport(int len, int S) {
    const int c = (len + S - 1) / S;
    return c < 1 ? 1 : c;
}
// photo rows the vertical pass can read: ymin >= y0 - ceil(support), ymax <= y0 + bh + ceil(support) + 1, clipped to the photo
__host__ __device__ inline void rs_rows(int H, int y0, int bh, int S, int* rbase, int* rows) {
    const int c = rs_csupport(bh, S);
    const int lo = y0 - c - 1 < 0 ? 0 : y0 - c - 1;
    const int hi = y0 + bh + c + 1 > H ? H : y0 + bh + c + 1;
    *rbase = lo;
    *rows = hi - lo;
}

// Bounds and integer coefficients of output index xx of one axis (input length n, box [in0, in0 + len), output S): Pillow's
// precompute_coeffs with the bilinear filter and normalize_coeffs_8bpc, in double, in its order of operations.  coef[0 .. ksize) gets
// the coefficients (zero past xmax - xmin); returns xmin, *cnt = xmax - xmin.  The weight is computed twice (sum, then quotient) from
// the same operands instead of being kept in a double array: the same value both times.
__device__ int rs_axis_coeffs(int n, int in0, int len, int S, int xx, int ksize, int* coef, int* cnt) {
#pragma clang fp contract(off)
    const double scale = (double)len / (double)S;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;
    const double ss = 1.0 / fs;
    const double center = (double)in0 + mkd_rounded(((double)xx + 0.5) * scale);
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n) xmax = n;
    xmax -= xmin;
    if (xmax > ksize) xmax = ksize;                      // (cannot happen: ksize = 2 ceil(support) + 1; keeps the table inside its row)
    if (xmax < 0) xmax = 0;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double a = mkd_rounded(((double)(x + xmin) - center + 0.5) * ss);
        if (a < 0.0) a = -a;
        const double w = a < 1.0 ? 1.0 - a : 0.0;
        ww += w;
    }
    for (int x = 0; x < xmax; ++x) {
        double a = mkd_rounded(((double)(x + xmin) - center + 0.5) * ss);
        if (a < 0.0) a = -a;
        double w = a < 1.0 ? 1.0 - a : 0.0;
        if (ww != 0.0) w = w / ww;
        coef[x] = (int)(0.5 + mkd_rounded(w * 4194304.0));           // no coefficient of this filter is negative
    }
    for (int x = xmax; x < ksize; ++x) coef[x] = 0;
    *cnt = xmax;
    return xmin;
}

__device__ __forceinline__ int rs_clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void resize_horizontal_kernel(const RsArgs a, int S, unsigned char* __restrict__ scratch) {
    __shared__ int coef[RS_G * RS_KMAX];
    __shared__ int xmin_s[RS_G], cnt_s[RS_G];
    const mkd_photo_desc d = a.d[blockIdx.z];
    int rbase, rows;
    rs_rows(d.H, d.y0, d.bh, S, &rbase, &rows);
    const int r0 = blockIdx.y * RS_ROWS;
    if (r0 >= rows) return;                              // (block-uniform, before the barrier)
    const int c0 = blockIdx.x * RS_G;
    const int ksize = 2 * rs_csupport(d.bw, S) + 1;
    if (threadIdx.x < RS_G && c0 + threadIdx.x < S)
        xmin_s[threadIdx.x] = rs_axis_coeffs(d.W, d.x0, d.bw, S, c0 + threadIdx.x, ksize, coef + threadIdx.x * RS_KMAX, cnt_s + threadIdx.x);
    __syncthreads();
    const int lc = threadIdx.x & (RS_G - 1), xx = c0 + lc;
    if (xx >= S) return;
    const int xmin = xmin_s[lc], cnt = cnt_s[lc];
    const int* ck = coef + lc * RS_KMAX;
    unsigned char* slab = scratch + a.off[blockIdx.z];
    const int rend = min(rows, r0 + RS_ROWS);
    for (int r = r0 + (threadIdx.x >> 5); r < rend; r += 256 / RS_G) {
        const unsigned char* p = d.pixels + (size_t)(rbase + r) * d.pitch_bytes + (size_t)xmin * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int k = 0; k < cnt; ++k) {
            const int c = ck[k];
            a0 += (int)p[3 * k] * c;
            a1 += (int)p[3 * k + 1] * c;
            a2 += (int)p[3 * k + 2] * c;
        }
        unsigned char* o = slab + ((size_t)r * S + xx) * 3;
        o[0] = (unsigned char)rs_clip8(a0);
        o[1] = (unsigned char)rs_clip8(a1);
        o[2] = (unsigned char)rs_clip8(a2);
    }
}

__global__ __launch_bounds__(256) void resize_vertical_kernel(const RsArgs a, int S, const unsigned char* __restrict__ scratch,
                                                              float* __restrict__ img01, unsigned char* __restrict__ u8_out,
                                                              unsigned char* __restrict__ labels_out) {
    __shared__ int coef[RS_GV * RS_KMAX];
    __shared__ int ymin_s[RS_GV], cnt_s[RS_GV];
    const int b = blockIdx.z;
    const mkd_photo_desc d = a.d[b];
    int rbase, rows;
    rs_rows(d.H, d.y0, d.bh, S, &rbase, &rows);
    const int y0o = blockIdx.y * RS_GV;
    const int ksize = 2 * rs_csupport(d.bh, S) + 1;
    if (threadIdx.x < RS_GV && y0o + threadIdx.x < S) {
        int cnt;
        int ymin = rs_axis_coeffs(d.H, d.y0, d.bh, S, y0o + threadIdx.x, ksize, coef + threadIdx.x * RS_KMAX, &cnt);
        // the rows are staged from rbase on; rs_rows covers every bound, so neither clamp acts
        if (ymin < rbase) ymin = rbase;
        if (ymin + cnt > rbase + rows) cnt = max(0, rbase + rows - ymin);
        ymin_s[threadIdx.x] = ymin - rbase;
        cnt_s[threadIdx.x] = cnt;
    }
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x;          // interleaved byte column: pixel x = e / 3, channel c = e - 3 x
    const int S3 = 3 * S;
    if (e >= S3) return;
    const int x = e / 3, c = e - 3 * x;
    const unsigned char* slab = scratch + a.off[b];
    const int ny = min(RS_GV, S - y0o);
    for (int i = 0; i < ny; ++i) {
        const int yy = y0o + i;
        const unsigned char* p = slab + (size_t)ymin_s[i] * S3 + e;
        const int* ck = coef + i * RS_KMAX;
        const int cnt = cnt_s[i];
        int acc = 1 << 21;
        for (int k = 0; k < cnt; ++k) acc += (int)p[(size_t)k * S3] * ck[k];
        const int v = rs_clip8(acc);
        if (u8_out) u8_out[((size_t)b * S + yy) * S3 + e] = (unsigned char)v;
        if (img01) img01[(((size_t)b * 3 + c) * S + yy) * S + x] = __fdiv_rn((float)v, 255.0f);
        if (labels_out && c == 0) {
            const int ly = d.y0 + ((2 * yy + 1) * d.bh) / (2 * S), lx = d.x0 + ((2 * x + 1) * d.bw) / (2 * S);
            labels_out[((size_t)b * S + yy) * S + x] = d.labels[(size_t)ly * d.W + lx];
        }
    }
}

__global__ __launch_bounds__(64) void resize_coeffs_kernel(int n, int in0, int len, int S, int ksize, int* __restrict__ bounds_out,
                                                           int* __restrict__ coef_out) {
    const int xx = blockIdx.x * 64 + threadIdx.x;
    if (xx >= S) return;
    int cnt;
    const int xmin = rs_axis_coeffs(n, in0, len, S, xx, ksize, coef_out + (size_t)xx * ksize, &cnt);
    bounds_out[2 * xx] = xmin;
    bounds_out[2 * xx + 1] = xmin + cnt;
}

// one axis of the paste's interpolation: the floor quotient (NOT clamped) and the weight of its upper neighbour
__device__ __forceinline__ int pp_axis_floor(int j, int len, int S, float* w) {
    const int num = (2 * j + 1) * S - len, den = 2 * len;            // |num| < 2^27
    int q = num / den;
    if (num < 0 && q * den != num) --q;                              // floor
    const int rem = num - q * den;                                   // 0 .. den - 1 <= 32767: exact in fp32
    *w = __fdiv_rn((float)rem, (float)den);
    return q;
}
// neighbours i0, i1 (clamped) and the weight of i1
__device__ __forceinline__ void pp_axis(int j, int len, int S, int* i0, int* i1, float* w) {
    const int q = pp_axis_floor(j, len, S, w);
    *i0 = min(max(q, 0), S - 1);
    *i1 = min(max(q + 1, 0), S - 1);
}
__device__ __forceinline__ float pp_lerp(float a, float b, float w) {
    return __fadd_rn(a, mkd_rounded(__fmul_rn(w, __fsub_rn(b, a))));
}

// WEIGHTED (mkd_paste_photo_weighted): the feather weight is multiplied by g, the bilinear sample of the photo-wide weight plane
// w [n][wh][ww] at the photo pixel (pp_axis on the photo's own axes); w, wh and ww are not read otherwise.
// GR >= 0 (mkd_paste_photo_guided, radius GR): u comes from gp_taps under the photo pixel's own luminance, inv = 1 / (256 sigma);
// GR = -1 is the bilinear paste and does not read inv.
template <bool WEIGHTED, int GR>
__global__ __launch_bounds__(256) void paste_photo_kernel(const PpArgs a, int S, const float* __restrict__ t, const float* __restrict__ s01,
                                                          int rho, const float* __restrict__ w, int wh, int ww, float inv) {
    const int b = blockIdx.z;
    const mkd_photo_desc d = a.d[b];
    const int j = blockIdx.x * PP_TW + (threadIdx.x & (PP_TW - 1));
    if (j >= d.bw) return;
    int x0i, x1i;
    float wx;
    pp_axis(j, d.bw, S, &x0i, &x1i, &wx);
    const int qx = GR >= 0 ? pp_axis_floor(j, d.bw, S, &wx) : 0;
    const int big = 1 << 30;
    int ex = big;
    if (d.x0 > 0) ex = j;
    if (d.x0 + d.bw < d.W) ex = min(ex, d.bw - 1 - j);
    const bool top_counts = d.y0 > 0, bottom_counts = d.y0 + d.bh < d.H;
    const float fr = (float)(rho + 1);
    int gx0 = 0, gx1 = 0;
    float ux = 0.0f;
    const float* wb = nullptr;
    if (WEIGHTED) {
        pp_axis(d.x0 + j, d.W, ww, &gx0, &gx1, &ux);
        wb = w + (size_t)b * wh * ww;
    }
    const size_t plane = (size_t)S * S;
    const float* tb = t + (size_t)b * 3 * plane;
    const float* sb = s01 + (size_t)b * 3 * plane;
    unsigned char* px = const_cast<unsigned char*>(d.pixels);
    const int i_end = min(d.bh, (int)(blockIdx.y + 1) * PP_TH);
    for (int i = blockIdx.y * PP_TH + (threadIdx.x >> 6); i < i_end; i += 256 / PP_TW) {
        int y0i, y1i;
        float wy;
        pp_axis(i, d.bh, S, &y0i, &y1i, &wy);
        const int qy = GR >= 0 ? pp_axis_floor(i, d.bh, S, &wy) : 0;
        int e = ex;
        if (top_counts) e = min(e, i);
        if (bottom_counts) e = min(e, d.bh - 1 - i);
        float al = __fdiv_rn((float)(min(e, rho) + 1), fr);                     // min(e + 1, rho + 1) without the overflow of big + 1
        if (WEIGHTED) {
            int gy0, gy1;
            float uy;
            pp_axis(d.y0 + i, d.H, wh, &gy0, &gy1, &uy);
            const float* r0 = wb + (size_t)gy0 * ww;
            const float* r1 = wb + (size_t)gy1 * ww;
            const float g = pp_lerp(pp_lerp(r0[gx0], r0[gx1], ux), pp_lerp(r1[gx0], r1[gx1], ux), uy);
            al = mkd_rounded(__fmul_rn(al, g));
        }
        unsigned char* p = px + (size_t)(d.y0 + i) * d.pitch_bytes + (size_t)(d.x0 + j) * 3;
        float u[3];
        if constexpr (GR >= 0) {
            gp_taps<float, GR>(tb, sb, S, qx, wx, qy, wy, (float)gp_luma(p[0], p[1], p[2]), inv, u);         // (the bytes are read before the writes below)
        } else {
            const int o00 = y0i * S + x0i, o01 = y0i * S + x1i, o10 = y1i * S + x0i, o11 = y1i * S + x1i;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* tc = tb + c * plane;
                const float* sc = sb + c * plane;
                const float d00 = pp_diff(tc[o00], sc[o00]), d01 = pp_diff(tc[o01], sc[o01]);
                const float d10 = pp_diff(tc[o10], sc[o10]), d11 = pp_diff(tc[o11], sc[o11]);
                const float top = pp_lerp(d00, d01, wx), bot = pp_lerp(d10, d11, wx);
                u[c] = pp_lerp(top, bot, wy);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float o = __fadd_rn((float)p[c], mkd_rounded(__fmul_rn(al, u[c])));
            p[c] = (unsigned char)fminf(fmaxf(rintf(o), 0.0f), 255.0f);
        }
    }
}

static_assert(MKD_PHOTO_MAX_BATCH == 16, "mkd_check_photo_descs (mkd_common.h) states the limit and its text as 16");
int check_descs(const char* what, const mkd_photo_desc* descs, int n, int S, bool need_labels) {
    const char* e = mkd_check_photo_descs(descs, n, S, need_labels, [S](const mkd_photo_desc& d) -> const char* {
        if (d.bw < 1 || d.bh < 1 || d.x0 < 0 || d.y0 < 0 || (int64_t)d.x0 + d.bw > d.W || (int64_t)d.y0 + d.bh > d.H)
            return "the box must be non-empty and lie inside the photo";
        if (d.bw > 32 * S || d.bh > 32 * S) return "the box must not exceed 32 S per side";
        return nullptr;
    });
    return e ? mkd_fail(MKD_ERR_ARG, std::string(what) + ": " + e) : 0;
}

size_t slab_bytes(const mkd_photo_desc& d, int S) {
    int rbase, rows;
    rs_rows(d.H, d.y0, d.bh, S, &rbase, &rows);
    return ((size_t)rows * S * 3 + 255) & ~(size_t)255;
}

template <int GR>
void launch_paste(const dim3 grid, hipStream_t stream, const PpArgs& a, int S, const float* t, const float* s01, int feather, const float* w,
                  int wh, int ww, float inv) {
    if (w)
        hipLaunchKernelGGL((paste_photo_kernel<true, GR>), grid, dim3(256), 0, stream, a, S, t, s01, feather, w, wh, ww, inv);
    else
        hipLaunchKernelGGL((paste_photo_kernel<false, GR>), grid, dim3(256), 0, stream, a, S, t, s01, feather, w, wh, ww, inv);
}

// the one launcher of the paste entries: w == nullptr is no weight plane, radius < 0 the bilinear paste (sigma is not read)
int paste_photo(const char* who, const mkd_photo_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w,
                int wh, int ww, int radius, float sigma, void* stream) {
    if (int rc = check_descs(who, descs, n, S, false)) return rc;
    if (!t || !s01) return mkd_fail(-1, std::string(who) + ": null t / s01");
    if (feather < 0 || feather > MKD_PHOTO_MAX_FEATHER) return mkd_fail(-1, std::string(who) + ": feather must be 0..64 photo pixels");
    if (w && (wh < 1 || ww < 1 || wh > 2048 || ww > 2048)) return mkd_fail(-1, std::string(who) + ": wh, ww must be 1..2048");
    if (radius >= 0)
        if (const char* e = gp_check(radius, sigma)) return mkd_fail(MKD_ERR_ARG, std::string(who) + ": " + e);
    const float inv = radius >= 0 ? 1.0f / (256.0f * sigma) : 0.0f;
    PpArgs a = {};
    int mw = 0, mh = 0;
    for (int i = 0; i < n; ++i) {
        a.d[i] = descs[i];
        mw = descs[i].bw > mw ? descs[i].bw : mw;
        mh = descs[i].bh > mh ? descs[i].bh : mh;
    }
    const dim3 grid((unsigned)((mw + PP_TW - 1) / PP_TW), (unsigned)((mh + PP_TH - 1) / PP_TH), (unsigned)n);      // y <= 1024
    switch (radius) {
        case 0: launch_paste<0>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv); break;
        case 1: launch_paste<1>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv); break;
        case 2: launch_paste<2>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv); break;
        default: launch_paste<-1>(grid, (hipStream_t)stream, a, S, t, s01, feather, w, wh, ww, inv);
    }
    MKD_LAUNCH_CHECK("paste_photo_kernel");
    return 0;
}

}  // namespace

extern "C" {

size_t mkd_crop_resize_scratch_bytes(const mkd_photo_desc* descs, int n, int S) {
    if (check_descs("mkd_crop_resize_scratch_bytes", descs, n, S, false)) return 0;
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += slab_bytes(descs[i], S);
    return total;
}

int mkd_crop_resize(const mkd_photo_desc* descs, int n, int S, float* img01, uint8_t* u8_out, uint8_t* labels_out, void* scratch,
                    void* stream) {
    if (int rc = check_descs("mkd_crop_resize", descs, n, S, labels_out != nullptr)) return rc;
    if (!img01 && !u8_out) return mkd_fail(-1, "mkd_crop_resize: img01 and u8_out are both null");
    if (!scratch || ((uintptr_t)scratch & 255)) return mkd_fail(-1, "mkd_crop_resize: the scratch must be a 256-byte aligned device buffer");
    RsArgs a = {};
    size_t off = 0;
    int max_rows = 0;
    for (int i = 0; i < n; ++i) {
        a.d[i] = descs[i];
        a.off[i] = off;
        off += slab_bytes(descs[i], S);
        int rbase, rows;
        rs_rows(descs[i].H, descs[i].y0, descs[i].bh, S, &rbase, &rows);
        max_rows = rows > max_rows ? rows : max_rows;
    }
    const dim3 gh((unsigned)((S + RS_G - 1) / RS_G), (unsigned)((max_rows + RS_ROWS - 1) / RS_ROWS), (unsigned)n);
    hipLaunchKernelGGL(resize_horizontal_kernel, gh, dim3(256), 0, (hipStream_t)stream, a, S, (unsigned char*)scratch);
    MKD_LAUNCH_CHECK("resize_horizontal_kernel");
    const dim3 gv((unsigned)((3 * S + 255) / 256), (unsigned)((S + RS_GV - 1) / RS_GV), (unsigned)n);
    hipLaunchKernelGGL(resize_vertical_kernel, gv, dim3(256), 0, (hipStream_t)stream, a, S, (const unsigned char*)scratch, img01, u8_out,
                       labels_out);
    MKD_LAUNCH_CHECK("resize_vertical_kernel");
    return 0;
}

int mkd_resize_coeffs(int N, int in0, int len, int S, int32_t* bounds_out, int32_t* coef_out, void* stream) {
    if (!bounds_out || !coef_out) return mkd_fail(-1, "mkd_resize_coeffs: null output");
    if (S < 8 || S > 1024 || N < 1 || N > 16384 || len < 1 || in0 < 0 || (int64_t)in0 + len > N || len > 32 * S)
        return mkd_fail(-1, "mkd_resize_coeffs: 8 <= S <= 1024, 1 <= N <= 16384, the box inside and at most 32 S long");
    const int ksize = 2 * rs_csupport(len, S) + 1;
    hipLaunchKernelGGL(resize_coeffs_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, (hipStream_t)stream, N, in0, len, S, ksize,
                       bounds_out, coef_out);
    MKD_LAUNCH_CHECK("resize_coeffs_kernel");
    return 0;
}

int mkd_paste_photo(const mkd_photo_desc* descs, int n, int S, const float* t, const float* s01, int feather, void* stream) {
    return paste_photo("mkd_paste_photo", descs, n, S, t, s01, feather, nullptr, 0, 0, -1, 0.0f, stream);
}

int mkd_paste_photo_weighted(const mkd_photo_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w,
                             int wh, int ww, void* stream) {
    if (!w) return mkd_fail(-1, "mkd_paste_photo_weighted: null w");
    if (wh < 1 || ww < 1 || wh > 2048 || ww > 2048) return mkd_fail(-1, "mkd_paste_photo_weighted: wh, ww must be 1..2048");
    return paste_photo("mkd_paste_photo_weighted", descs, n, S, t, s01, feather, w, wh, ww, -1, 0.0f, stream);
}

int mkd_paste_photo_guided(const mkd_photo_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w, int wh,
                           int ww, int radius, float sigma, void* stream) {
    if (radius < 0) return mkd_fail(MKD_ERR_ARG, std::string("mkd_paste_photo_guided: ") + gp_check(radius, sigma));
    return paste_photo("mkd_paste_photo_guided", descs, n, S, t, s01, feather, w, wh, ww, radius, sigma, stream);
}

}  // extern "C"
