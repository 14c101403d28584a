// Video clips (include/mkd.h: mkd_motion_warp): block-matched motion for the temporal makeup filter.  mkd_temporal_diff compares pixel p
// of this frame with pixel p of the previous one; a mouth that opens or a crop that lags the face by a pixel moves the picture under p
// and the filter restarts exactly where lipstick and eye shadow sit.  As a video codec does, this kernel finds ONE integer displacement
// per block of model pixels between the previous frame's luminance (the Y pool) and this frame's (formed from s01) and fetches the
// previous state (D and Y) through it into a third pair of pools, which mkd_temporal_diff then reads as its _in pools, unchanged.
//
// One workgroup of 256 threads per 16 x 16 pixel tile: one block at block = 16, four at block = 8.  The tile's luminance and the
// previous luminance of the tile plus a halo of `search` pixels are staged in LDS as integers (replicated edges are staged as such, so
// a clamped fetch is a plain LDS read).  The C = (2 search + 1)^2 candidates are spread over threads, neighbouring threads on
// neighbouring vx; where C is small the rows of a block are split over min(block, 256 / C) groups of C threads.  The sums of absolute
// differences are integers, so any order gives the same bits.  Partial sums meet in LDS, every candidate becomes one packed 64-bit key
// (cost, |vy| + |vx|, vy, vx), the minimum goes through wave shuffles and then through LDS across the four waves, and all threads do
// the warp copy of their own pixel.  Three barriers, all reached by every thread of the workgroup: a face without a previous frame
// leaves as a whole workgroup before the first one (the slot is a kernel argument indexed by blockIdx.z).
#include "mkd_common.h"
#include "paste_guided.h"
#include "../../include/mkd.h"

namespace {

constexpr int MW_T = 16;                                  // tile side
constexpr int MW_THREADS = MW_T * MW_T;
constexpr int MW_SMAX = 7;                                // largest search
constexpr int MW_HMAX = MW_T + 2 * MW_SMAX;               // tile plus halo
constexpr int MW_WAVES = MW_THREADS / 64;

struct MwArgs {
    int32_t slot[MKD_PHOTO_MAX_BATCH];
};

__device__ __forceinline__ unsigned long long mw_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

template <int BLK>
__global__ __launch_bounds__(MW_THREADS) void motion_warp_kernel(const MwArgs a, int S, const float* __restrict__ s01,
                                                                  const float* __restrict__ D_in, const float* __restrict__ Y_in, int search,
                                                                  int penalty, float* __restrict__ D_w, float* __restrict__ Y_w,
                                                                  int32_t* __restrict__ vec_out) {
    constexpr int NB = MW_T / BLK;                        // blocks per tile side
    constexpr int NBT = NB * NB;
    __shared__ int y_cur[MW_T * MW_T];
    __shared__ int y_old[MW_HMAX * MW_HMAX];
    __shared__ int part_sad[NBT * MW_THREADS];            // [block of the tile][group of rows][candidate], groups * C <= 256
    __shared__ unsigned long long wave_key[MW_WAVES * NBT];
    const int b = blockIdx.z;
    const int slot = a.slot[b];
    const int ty0 = blockIdx.y * MW_T, tx0 = blockIdx.x * MW_T;
    const int lx = threadIdx.x % MW_T, ly = threadIdx.x / MW_T;
    const int x = tx0 + lx, y = ty0 + ly;
    const int nb = (S + BLK - 1) / BLK;
    const bool inside = x < S && y < S;
    const bool corner = inside && lx % BLK == 0 && ly % BLK == 0;          // the thread that reports its block's vector
    int32_t* vo = vec_out ? vec_out + (((size_t)b * nb + y / BLK) * nb + x / BLK) * 2 : nullptr;
    if (slot < 0) {          // (uniform over the workgroup, before any barrier) no previous frame: zero vectors, no pool is touched
        if (corner && vo) vo[0] = vo[1] = 0;
        return;
    }
    const size_t plane = (size_t)S * S;
    const float* sb = s01 + (size_t)b * 3 * plane;
    const float* yi = Y_in + (size_t)slot * plane;
    const int HW = MW_T + 2 * search;
    {
        const int gy = gp_clampi(y, 0, S - 1), gx = gp_clampi(x, 0, S - 1);
        const size_t o = (size_t)gy * S + gx;
        y_cur[threadIdx.x] = gp_luma(gp_byte(sb[o]), gp_byte(sb[plane + o]), gp_byte(sb[2 * plane + o]));
    }
    for (int e = threadIdx.x; e < HW * HW; e += MW_THREADS) {
        const int gy = gp_clampi(ty0 + e / HW - search, 0, S - 1), gx = gp_clampi(tx0 + e % HW - search, 0, S - 1);
        y_old[e] = (int)yi[(size_t)gy * S + gx];
    }
    __syncthreads();
    // the sums of absolute differences: thread = (group of rows, candidate)
    const int side = 2 * search + 1, C = side * side;
    const int groups = min(BLK, MW_THREADS / C);
    const int cand = threadIdx.x % C, grp = threadIdx.x / C;
    const int vh = min(MW_T, S - ty0), vw = min(MW_T, S - tx0);          // the rows and columns of the tile inside the image
    if (grp < groups) {
        const int* old = y_old + (cand / side) * HW + cand % side;       // (py + vy + search) * HW + px + vx + search at p = 0
#pragma unroll
        for (int by = 0; by < NB; ++by) {
            int sad[NB];
#pragma unroll
            for (int bx = 0; bx < NB; ++bx) sad[bx] = 0;
            const int r1 = min((by + 1) * BLK, vh);
            for (int r = by * BLK + grp; r < r1; r += groups) {
                const int* cr = y_cur + r * MW_T;
                const int* orow = old + r * HW;
#pragma unroll
                for (int c = 0; c < MW_T; ++c)
                    if (c < vw) sad[c / BLK] += abs(cr[c] - orow[c]);
            }
#pragma unroll
            for (int bx = 0; bx < NB; ++bx) part_sad[((by * NB + bx) * groups + grp) * C + cand] = sad[bx];
        }
    }
    __syncthreads();
    // one key per candidate and block, the minimum over the wave, then over the waves
    const int vy = cand / side - search, vx = cand % side - search;
    const int l1 = abs(vy) + abs(vx);
#pragma unroll
    for (int k = 0; k < NBT; ++k) {
        unsigned long long key = ~0ull;
        if (threadIdx.x < C) {
            const int bh = min(BLK, vh - (k / NB) * BLK), bw = min(BLK, vw - (k % NB) * BLK);
            if (bh > 0 && bw > 0) {
                int cost = penalty * (bh * bw) * l1;                     // <= 65280 * 256 * 14
                for (int g = 0; g < groups; ++g) cost += part_sad[(k * groups + g) * C + cand];
                key = ((unsigned long long)(unsigned)cost << 12) | (unsigned)(l1 << 8) | (unsigned)((vy + MW_SMAX) << 4) | (unsigned)(vx + MW_SMAX);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) key = mw_min(key, (unsigned long long)__shfl_xor((long long)key, off));
        if (threadIdx.x % 64 == 0) wave_key[(threadIdx.x / 64) * NBT + k] = key;
    }
    __syncthreads();
    if (!inside) return;          // (after the last barrier)
    const int k = (ly / BLK) * NB + lx / BLK;
    unsigned long long key = wave_key[k];
#pragma unroll
    for (int w = 1; w < MW_WAVES; ++w) key = mw_min(key, wave_key[w * NBT + k]);
    const int bvy = (int)((key >> 4) & 15) - MW_SMAX, bvx = (int)(key & 15) - MW_SMAX;
    if (corner && vo) {
        vo[0] = bvy;
        vo[1] = bvx;
    }
    // the warp copy: the bits of the previous state at q = clamp(p + v)
    const size_t o = (size_t)y * S + x;
    const size_t q = (size_t)gp_clampi(y + bvy, 0, S - 1) * S + gp_clampi(x + bvx, 0, S - 1);
    const uint32_t* din = reinterpret_cast<const uint32_t*>(D_in) + (size_t)slot * 3 * plane;
    uint32_t* dw = reinterpret_cast<uint32_t*>(D_w) + (size_t)slot * 3 * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) dw[c * plane + o] = din[c * plane + q];
    reinterpret_cast<uint32_t*>(Y_w)[(size_t)slot * plane + o] = reinterpret_cast<const uint32_t*>(Y_in)[(size_t)slot * plane + q];
}

bool mw_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace

extern "C" {

int mkd_motion_warp(const float* s01, int n, int S, const float* D_in, const float* Y_in, const int32_t* slot_in, int pool, int search, int block,
                    int penalty, float* D_w, float* Y_w, int32_t* vec_out, void* stream) {
    const std::string who = "mkd_motion_warp: ";
    if (!s01 || !D_in || !Y_in || !slot_in || !D_w || !Y_w) return mkd_fail(MKD_ERR_ARG, who + "null pointer");
    if (n < 1 || n > MKD_PHOTO_MAX_BATCH) return mkd_fail(MKD_ERR_ARG, who + "1..16 faces per call");
    if (S < 8 || S > 1024) return mkd_fail(MKD_ERR_ARG, who + "S must be 8..1024");
    if (search < 1 || search > MW_SMAX) return mkd_fail(MKD_ERR_ARG, who + "search must be 1..7");
    if (block != 8 && block != 16) return mkd_fail(MKD_ERR_ARG, who + "block must be 8 or 16");
    if (penalty < 0 || penalty > 65280) return mkd_fail(MKD_ERR_ARG, who + "penalty must be 0..65280");
    if (pool < 1 || pool > 65536) return mkd_fail(MKD_ERR_ARG, who + "pool must hold 1..65536 slots");
    MwArgs a = {};
    for (int i = 0; i < n; ++i) {
        if (slot_in[i] < -1 || slot_in[i] >= pool) return mkd_fail(MKD_ERR_ARG, who + "slot_in must be -1 or a slot of the pool");
        for (int j = 0; j < i; ++j)
            if (slot_in[i] >= 0 && slot_in[j] == slot_in[i]) return mkd_fail(MKD_ERR_ARG, who + "a slot must not repeat in slot_in");
        a.slot[i] = slot_in[i];
    }
    const size_t yb = (size_t)pool * S * S * sizeof(float), db = 3 * yb, sbytes = (size_t)n * 3 * S * S * sizeof(float);
    if (mw_overlap(D_w, db, D_in, db) || mw_overlap(D_w, db, Y_in, yb) || mw_overlap(D_w, db, s01, sbytes) || mw_overlap(Y_w, yb, D_in, db) ||
        mw_overlap(Y_w, yb, Y_in, yb) || mw_overlap(Y_w, yb, s01, sbytes) || mw_overlap(D_w, db, Y_w, yb))
        return mkd_fail(MKD_ERR_ARG, who + "D_w and Y_w must not overlap D_in, Y_in, s01 or each other");
    const unsigned tiles = (unsigned)((S + MW_T - 1) / MW_T);
    const dim3 grid(tiles, tiles, (unsigned)n);
    if (block == 8)
        hipLaunchKernelGGL((motion_warp_kernel<8>), grid, dim3(MW_THREADS), 0, (hipStream_t)stream, a, S, s01, D_in, Y_in, search, penalty, D_w, Y_w,
                           vec_out);
    else
        hipLaunchKernelGGL((motion_warp_kernel<16>), grid, dim3(MW_THREADS), 0, (hipStream_t)stream, a, S, s01, D_in, Y_in, search, penalty, D_w, Y_w,
                           vec_out);
    MKD_LAUNCH_CHECK("motion_warp_kernel");
    return 0;
}

}  // extern "C"
