// Region ids, window counts and blend weights of the teacher kernels (mkd_pgt_compose, mkd_pgt_warp; include/mkd.h has the definition):
//   id(p)  = the first of lip (1), eye_left (2), eye_right (3), skin (4) whose mask is non-zero at p, else 0
//   c_r(p) = the pixels q of the (2 F + 1)^2 window around p that lie inside the image and have id(q) = r
//   weight = a_r * (c_r / K), K = (2 F + 1)^2, in double, each operation rounded on its own; c_r = 0 gives +0
// One workgroup of 256 threads per 16 x 16 tile: the ids of the tile plus its halo sit in LDS at a byte per pixel, and the four counts are
// separable sums (rows, then columns) carried as 4 x 16 bits of one 64-bit word (a row sum is <= 17, a total <= 289).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

constexpr int PG_T = 16;                       // tile side
constexpr int PG_MAXF = 8;                     // feather limit: the staged plane is at most 32 x 32
constexpr int PG_R = PG_T + 2 * PG_MAXF;       // row stride of the id plane

__device__ __forceinline__ int pg_mask_plane(int r) { return r == 0 ? 0 : r == 1 ? 2 : r == 2 ? 3 : 1; }      // id r + 1 -> plane of (lip, skin, eye_left, eye_right)
__device__ __forceinline__ int pg_id(unsigned lip, unsigned skin, unsigned eye_l, unsigned eye_r) { return lip ? 1 : eye_l ? 2 : eye_r ? 3 : skin ? 4 : 0; }

// ids[PG_R * PG_R]: the ids of the (16 + 2 F)^2 pixels around the tile at (ty0, tx0); outside the image is 0.  mk: this sample's lip
// plane, the other planes `plane` bytes apart.  The caller syncs before pg_row_counts.
__device__ __forceinline__ void pg_stage_ids(const uint8_t* __restrict__ mk, size_t plane, int H, int W, int F, int ty0, int tx0, int tid, uint8_t* ids) {
    const int R = PG_T + 2 * F;
    for (int i = tid; i < R * R; i += 256) {
        const int ly = i / R, lx = i - ly * R, gy = ty0 - F + ly, gx = tx0 - F + lx;
        int id = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t p = (size_t)gy * W + gx;
            id = pg_id(mk[p], mk[plane + p], mk[2 * plane + p], mk[3 * plane + p]);
        }
        ids[ly * PG_R + lx] = (uint8_t)id;
    }
}

// rows[PG_R * PG_T]: the packed counts of the 2 F + 1 ids to the right of each staged pixel.  The caller syncs before pg_window_counts.
__device__ __forceinline__ void pg_row_counts(const uint8_t* ids, int F, int tid, unsigned long long* rows) {
    const int R = PG_T + 2 * F;
    for (int i = tid; i < R * PG_T; i += 256) {
        const int ly = i >> 4, x = i & 15;
        unsigned long long s = 0;
        for (int k = 0; k <= 2 * F; ++k) {
            const int id = ids[ly * PG_R + x + k];
            s += id ? 1ull << (16 * (id - 1)) : 0ull;
        }
        rows[ly * PG_T + x] = s;
    }
}

// the packed counts c_1 .. c_4 of tile pixel tid = 16 y + x
__device__ __forceinline__ unsigned long long pg_window_counts(const unsigned long long* rows, int F, int tid) {
    const int y = tid >> 4, x = tid & 15;
    unsigned long long s = 0;
    for (int k = 0; k <= 2 * F; ++k) s += rows[(y + k) * PG_T + x];
    return s;
}

__device__ __forceinline__ int pg_count(unsigned long long s, int r) { return (int)((s >> (16 * r)) & 0xffffull); }

__device__ __forceinline__ double pg_weight(float a, int c, double K) {
#pragma clang fp contract(off)
    return c ? (double)a * ((double)c / K) : 0.0;
}
