// The histogram-matching teacher (mkd_pgt_compose; include/mkd.h holds the definition, tests/teacher_ref.py restates it): EleGANt's
// pseudo ground truth (reference teacher.py:96-112) at warp weight alpha = 0, i.e. region-wise histogram matching of the source to
// the reference, composed into ONE image.  BUILD-DEFINED where the reference leaves it open (region priority, feather, border).
//
//   id(p)    = the first of lip (1), eye_left (2), eye_right (3), skin (4) whose mask is non-zero at p, else 0
//   c_r(p)   = the pixels q of the (2 F + 1)^2 window around p that lie inside the image and have id(q) = r;  K = (2 F + 1)^2
//   v        = clamp(s_c, 0, 1) * 255 (fp32, one rounding; a zero is +0), i = min(int(v), 255): mkd_hist_match's value and bin
//   out_c(p) = clamp((v + sum_{r = 1..4} (a_r * (c_r / K)) * (T_{r,c}[i] - i)) / 255, 0, 1)
// in double from the fp32 / integer operands, every operation rounded on its own (nothing contracts), the terms added in the order
// r = 1..4, and ONE rounding to fp32 at the end.  A pixel whose window holds no region skips the sum: its terms are all +-0.
//
// One workgroup per 16 x 16 output tile.  F > 0: the region ids of the tile plus its halo go to LDS at a byte per pixel, the four
// counts are separable sums (rows, then columns) carried as 4 x 16 bits of one 64-bit word (a row sum is <= 17, a total <= 289), and
// the weights a_r c_r / K go back to LDS as doubles, because the 16-byte form below gives a lane other pixels than the count pass
// (ids, counts and weights: pgt_regions.h, shared with mkd_pgt_warp).  F = 0 stages nothing but the tables: id(p) comes straight from the masks.
#include "mkd_common.h"
#include "pgt_regions.h"
#include "../../include/mkd.h"

namespace {

constexpr int PG_TAB = 3 * 256;                // one region's tables

struct PgWeights { double w[4]; };

// tab: this channel's 256 entries of region id 1; the other regions follow at PG_TAB each
__device__ __forceinline__ float pg_value(float s, const PgWeights& g, const uint8_t* tab) {
#pragma clang fp contract(off)
    const float v = hm_value(s) + 0.0f;          // (+ 0: a source of -0 gives +0 whatever zero fmaxf picks; every other value is unchanged)
    double acc = (double)v;
    if (g.w[0] != 0.0 || g.w[1] != 0.0 || g.w[2] != 0.0 || g.w[3] != 0.0) {
        const int i = hm_bin(v);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = acc + g.w[r] * (double)((int)tab[r * PG_TAB + i] - i);
    }
    const double o = acc / 255.0;
    return (float)fmin(fmax(o, 0.0), 1.0);
}

__device__ __forceinline__ PgWeights pg_hard_weights(int id, const float* a) {          // F = 0: c_r / K is 0 or 1
    PgWeights g;
#pragma unroll
    for (int r = 0; r < 4; ++r) g.w[r] = id == r + 1 ? (double)a[r] : 0.0;
    return g;
}

// grid (tiles_x * tiles_y, n).  VEC: W % 4 == 0, src / out 16-byte aligned (and masks 4-byte aligned when !HALO): wave c < 3 writes
// channel c of the tile, a lane four pixels of a row with one 16-byte load and store; else a thread is a pixel and walks the channels.
template <bool VEC, bool HALO>
__global__ __launch_bounds__(256) void pgt_compose_kernel(const float* __restrict__ src, const uint8_t* __restrict__ masks,
                                                          const uint8_t* __restrict__ tables, const float* __restrict__ strengths, int n, int H,
                                                          int W, int F, int tiles_x, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[4 * PG_TAB];
    __shared__ uint8_t ids[HALO ? PG_R * PG_R : 1];
    __shared__ unsigned long long rows[HALO ? PG_R * PG_T : 1];
    __shared__ double wgt[HALO ? 4 * PG_T * PG_T : 1];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * PG_T, tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * PG_T;
    const size_t HW = (size_t)H * W, plane = (size_t)n * HW;
    const uint8_t* mk = masks + (size_t)b * HW;

    if (((uintptr_t)tables & 3) == 0) {
        for (int i = tid; i < 4 * PG_TAB / 4; i += 256) {
            const int r = i / (PG_TAB / 4);
            ((uint32_t*)tab)[i] = ((const uint32_t*)(tables + ((size_t)pg_mask_plane(r) * n + b) * PG_TAB))[i - r * (PG_TAB / 4)];
        }
    } else {
        for (int i = tid; i < 4 * PG_TAB; i += 256) {
            const int r = i / PG_TAB;
            tab[i] = tables[((size_t)pg_mask_plane(r) * n + b) * PG_TAB + (i - r * PG_TAB)];
        }
    }
    float a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = strengths ? strengths[(size_t)b * 4 + pg_mask_plane(r)] : 1.0f;

    if (HALO) {
        pg_stage_ids(mk, plane, H, W, F, ty0, tx0, tid, ids);
        __syncthreads();
        pg_row_counts(ids, F, tid, rows);
        __syncthreads();
        const unsigned long long s = pg_window_counts(rows, F, tid);
        const double K = (double)((2 * F + 1) * (2 * F + 1));
#pragma unroll
        for (int r = 0; r < 4; ++r) wgt[r * 256 + tid] = pg_weight(a[r], pg_count(s, r), K);
    }
    __syncthreads();

    if (VEC) {
        const int c = tid >> 6, lane = tid & 63, y = lane >> 2, x = (lane & 3) * 4, gy = ty0 + y, gx = tx0 + x;
        if (c >= 3 || gy >= H || gx >= W) return;          // W % 4 == 0: a group of four is inside or outside as a whole
        const size_t p = (size_t)gy * W + gx, e = ((size_t)b * 3 + c) * HW + p;
        const f32x4 s = *(const f32x4*)(src + e);
        uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
        if (!HALO) { m0 = *(const uint32_t*)(mk + p); m1 = *(const uint32_t*)(mk + plane + p); m2 = *(const uint32_t*)(mk + 2 * plane + p); m3 = *(const uint32_t*)(mk + 3 * plane + p); }
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            PgWeights g;
            if (HALO) {
#pragma unroll
                for (int r = 0; r < 4; ++r) g.w[r] = wgt[r * 256 + y * PG_T + x + k];
            } else {
                g = pg_hard_weights(pg_id((m0 >> (8 * k)) & 0xffu, (m1 >> (8 * k)) & 0xffu, (m2 >> (8 * k)) & 0xffu, (m3 >> (8 * k)) & 0xffu), a);
            }
            o[k] = pg_value(s[k], g, tab + c * 256);
        }
        *(f32x4*)(out + e) = o;
    } else {
        const int y = tid >> 4, x = tid & 15, gy = ty0 + y, gx = tx0 + x;
        if (gy >= H || gx >= W) return;
        const size_t p = (size_t)gy * W + gx;
        PgWeights g;
        if (HALO) {
#pragma unroll
            for (int r = 0; r < 4; ++r) g.w[r] = wgt[r * 256 + tid];
        } else {
            g = pg_hard_weights(pg_id(mk[p], mk[plane + p], mk[2 * plane + p], mk[3 * plane + p]), a);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t e = ((size_t)b * 3 + c) * HW + p;
            out[e] = pg_value(src[e], g, tab + c * 256);
        }
    }
}

inline bool pg_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

int mkd_pgt_launches(void) { return 1; }

int mkd_pgt_compose(const float* src, const uint8_t* masks, const uint8_t* tables, const float* strengths, int n, int H, int W, int feather,
                    float* out, void* stream) {
    const std::string who = "mkd_pgt_compose: ";
    if (!src || !masks || !tables || !out) return mkd_fail(MKD_ERR_ARG, who + "null src / masks / tables / out");
    if (n < 1 || n > 65535 || H < 1 || W < 1 || (int64_t)H * W > (1 << 24))
        return mkd_fail(MKD_ERR_ARG, who + "1 <= n <= 65535 images of [3, H, W] with H * W <= 2^24");
    if (feather < 0 || feather > PG_MAXF) return mkd_fail(MKD_ERR_ARG, who + "feather must be 0..8");
    if (!pg_aligned(src, 4) || !pg_aligned(out, 4) || (strengths && !pg_aligned(strengths, 4)))
        return mkd_fail(MKD_ERR_ARG, who + "fp32 arrays must be 4-byte aligned");
    const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out, bytes = (uintptr_t)n * 3 * (uintptr_t)H * (uintptr_t)W * sizeof(float);
    if (s0 < o0 + bytes && o0 < s0 + bytes) return mkd_fail(MKD_ERR_ARG, who + "out may not overlap src");
    const int tiles_x = (W + PG_T - 1) / PG_T, tiles_y = (H + PG_T - 1) / PG_T;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n), block(256);
    const bool halo = feather > 0;
    const bool vec = W % 4 == 0 && pg_aligned(src, 16) && pg_aligned(out, 16) && (halo || pg_aligned(masks, 4));
#define PG_LAUNCH(V, Hl) hipLaunchKernelGGL((pgt_compose_kernel<V, Hl>), grid, block, 0, (hipStream_t)stream, src, masks, tables, strengths, n, H, W, \
                                            feather, tiles_x, out)
    if (vec && halo) PG_LAUNCH(true, true);
    else if (vec) PG_LAUNCH(true, false);
    else if (halo) PG_LAUNCH(false, true);
    else PG_LAUNCH(false, false);
#undef PG_LAUNCH
    MKD_LAUNCH_CHECK("pgt_compose_kernel");
    return 0;
}
