// Connected components of a label map (include/mkd.h: mkd_label_components): the 8-connected sets of the pixels whose label is in a
// class set, with per-component id (smallest linear index), area and bounding box, the largest max_out of them as a table.  Integer
// arithmetic only: the outputs do not depend on launch geometry or arrival order.  Context-free; the call only enqueues, four
// launches whatever the data.  No workgroup waits for another: what one phase needs from another is separated by a kernel boundary.
//
// parent[] is a union-find forest over linear pixel indices of one image with the invariant parent[i] <= i for in-pixels (-1 marks an
// out-pixel), so a root is the smallest index of its set and every walk towards a root strictly decreases.
//   1. cc_tile_kernel: one CC_T x CC_T tile per workgroup.  Union-find in LDS over the tile's own pixel pairs (lock-free atomicMin
//      merge, Komura 2015 / Playne-Hawick 2018), then parent[i] = the tile-local root as a GLOBAL index, for every pixel of the image
//      (the scratch's earlier contents never matter).  Local roots get their statistics slots cleared; tile 0 clears the root counter.
//   2. cc_seam_kernel: one thread per pixel on the first column / row of a tile; unions it with its three neighbours across the seam.
//   3. cc_stats_kernel: per tile, the pixels' area and box are summed per tile-local root in LDS, then ONE thread per local root
//      walks to the final root and adds the partial sums there (integer atomicAdd / atomicMin / atomicMax: exact in any order); final
//      roots append themselves to the image's root list (the ORDER of that list is arrival-dependent, nothing read from it is).
//   4. cc_select_kernel: one workgroup per image: keys (area << 32) | ~id of the roots with area >= min_area, then max_out rounds of a
//      block-wide maximum below the previous round's key: area descending, ties by id ascending.
// Further down: mkd_owner_map (the nearest table component of every pixel, two launches) and mkd_owner_weights (its window fractions).
#include "mkd_common.h"
#include "../../include/mkd.h"

#include <limits.h>

namespace {

constexpr int CC_T = 32;                 // tile side; CC_T * CC_T pixels per workgroup
constexpr int CC_PIX = CC_T * CC_T;
constexpr int CC_NT = 256;               // threads of the tile kernels: 4 pixels each
constexpr int CC_SEL_NT = 512;           // threads of the selection kernel
constexpr int CC_MAX_OUT = 64;
constexpr int CC_HDR = 64;               // int32 words in front of an image's arrays (word 0: the root counter), keeps them 256-byte aligned

static_assert(sizeof(mkd_component) == 24, "mkd_component is six int32");

// int32 words of one image's scratch: header, parent, area, r0, r1, c0, c1 [HW each], root list [cap], keys [cap] uint64.
// cap = ceil(H / 2) * ceil(W / 2): two in-pixels of one aligned 2 x 2 block are 8-adjacent, so a block holds at most one root
__host__ __device__ inline size_t cc_cap(int H, int W) { return (size_t)((H + 1) / 2) * (size_t)((W + 1) / 2); }
__host__ __device__ inline size_t cc_words(int H, int W) {
    const size_t hw = (size_t)H * (size_t)W;
    const size_t w = CC_HDR + 6 * hw + 3 * cc_cap(H, W) + 2;          // (+ 2: the keys start on an even word)
    return (w + 63) / 64 * 64;
}
struct CcImage {
    int* hdr; int* parent; int* area; int* r0; int* r1; int* c0; int* c1; int* list; unsigned long long* keys;
};
__device__ __forceinline__ CcImage cc_image(void* scratch, int b, int H, int W) {
    const size_t hw = (size_t)H * (size_t)W, cap = cc_cap(H, W);
    int* p = (int*)scratch + (size_t)b * cc_words(H, W);
    CcImage im;
    im.hdr = p;
    im.parent = p + CC_HDR;
    im.area = im.parent + hw;
    im.r0 = im.area + hw;
    im.r1 = im.r0 + hw;
    im.c0 = im.r1 + hw;
    im.c1 = im.c0 + hw;
    im.list = im.c1 + hw;
    size_t k = CC_HDR + 6 * hw + cap;
    k += k & 1;
    im.keys = (unsigned long long*)(p + k);
    return im;
}

__device__ __forceinline__ bool cc_in(uint8_t l, uint64_t classes) { return l < 64 && ((classes >> l) & 1ull); }

// ---- union-find in LDS (workgroup scope) ------------------------------------------------------------------------------------------
// Bound: L[i] <= i always (entries only ever receive smaller values, by atomicMin), so i strictly decreases: at most CC_PIX steps.
__device__ __forceinline__ int cc_find_lds(int* L, int i) {
    for (;;) {
        const int p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == i) return i;
        i = p;
    }
}
// Bound: a round repeats only when atomicMin found L[hi] != hi, i.e. another thread lowered that entry after our find; entries are
// non-negative and only decrease, so the workgroup's lowerings, and with them the repeats, are finite.  When the atomicMin replaced a
// link hi -> old by hi -> lo, the next round unions old with lo: no link is ever lost.
__device__ __forceinline__ void cc_union_lds(int* L, int a, int b) {
    for (;;) {
        a = cc_find_lds(L, a);
        b = cc_find_lds(L, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(&L[hi], lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}
// ---- the same on the global forest (agent scope) ----------------------------------------------------------------------------------
// Bound: parent[i] <= i for in-pixels and the walk only visits in-pixels, so i strictly decreases: at most H * W steps.
__device__ __forceinline__ int cc_find(int* parent, int i) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == i) return i;
        i = p;
    }
}
// Bound: as cc_union_lds -- a repeat needs another thread to have lowered parent[hi] since our find, and the entries of the image,
// bounded below by 0, only decrease.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(&parent[hi], lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// launch 1 -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_NT) void cc_tile_kernel(const uint8_t* __restrict__ labels, int H, int W, int ntx, uint64_t classes,
                                                        void* scratch) {
    __shared__ int L[CC_PIX];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / ntx) * CC_T, tx0 = (tile % ntx) * CC_T;
    const CcImage im = cc_image(scratch, b, H, W);
    const uint8_t* lab = labels + (size_t)b * H * W;
    if (tile == 0 && threadIdx.x == 0) im.hdr[0] = 0;
#pragma unroll
    for (int k = 0; k < CC_PIX / CC_NT; ++k) {
        const int li = threadIdx.x + k * CC_NT, y = ty0 + li / CC_T, x = tx0 + li % CC_T;
        L[li] = (y < H && x < W && cc_in(lab[(size_t)y * W + x], classes)) ? li : -1;
    }
    __syncthreads();
    // Unions over the tile's own pairs.  Whether an entry is >= 0 never changes, so "is a neighbour in" may be read while others merge.
    // With the pixel above in, its link alone suffices: by induction over the rows, horizontally adjacent in-pixels of a row end up
    // in one set (row 0 of the tile links them directly; further down either the left link is made, or both have the pixel above in
    // and those two are adjacent in the row above, or the left one links to its upper right, which is the pixel above), and that
    // connects the left and both diagonal neighbours through the pixel above.
#pragma unroll
    for (int k = 0; k < CC_PIX / CC_NT; ++k) {
        const int li = threadIdx.x + k * CC_NT, ly = li / CC_T, lx = li % CC_T;
        if (__hip_atomic_load(&L[li], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 0) continue;
        auto in = [&](int j) { return __hip_atomic_load(&L[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0; };
        if (ly > 0 && in(li - CC_T)) {
            cc_union_lds(L, li, li - CC_T);
        } else {
            if (lx > 0 && in(li - 1)) cc_union_lds(L, li, li - 1);
            if (ly > 0 && lx > 0 && in(li - CC_T - 1)) cc_union_lds(L, li, li - CC_T - 1);
            if (ly > 0 && lx < CC_T - 1 && in(li - CC_T + 1)) cc_union_lds(L, li, li - CC_T + 1);
        }
    }
    __syncthreads();
    // nothing writes L any more.  Row-major order is the same in the tile and in the image, so the local root is the set's smallest
    // global index inside the tile and parent[i] <= i holds
#pragma unroll
    for (int k = 0; k < CC_PIX / CC_NT; ++k) {
        const int li = threadIdx.x + k * CC_NT, y = ty0 + li / CC_T, x = tx0 + li % CC_T;
        if (y >= H || x >= W) continue;
        const int g = y * W + x;
        if (L[li] < 0) {
            im.parent[g] = -1;
            continue;
        }
        const int r = cc_find_lds(L, li);
        im.parent[g] = (ty0 + r / CC_T) * W + tx0 + r % CC_T;
        if (r == li) {          // every final root is one of these
            im.area[g] = 0;
            im.r0[g] = INT_MAX;
            im.r1[g] = -1;
            im.c0[g] = INT_MAX;
            im.c1[g] = -1;
        }
    }
}

// launch 2 -----------------------------------------------------------------------------------------------------------------------------
// index k < nV: pixel (x = s CC_T, y) of vertical seam s = 1 + k / H; else pixel (x, y = s CC_T) of horizontal seam s = 1 + (k - nV) / W
__global__ __launch_bounds__(CC_NT) void cc_seam_kernel(int H, int W, int nV, int nH, void* scratch) {
    const int k = blockIdx.x * CC_NT + threadIdx.x;
    if (k >= nV + nH) return;
    const CcImage im = cc_image(scratch, blockIdx.y, H, W);
    int* parent = im.parent;
    int x, y, nx[3], ny[3];
    if (k < nV) {
        x = (1 + k / H) * CC_T;
        y = k % H;
        for (int j = 0; j < 3; ++j) { nx[j] = x - 1; ny[j] = y - 1 + j; }
    } else {
        const int q = k - nV;
        y = (1 + q / W) * CC_T;
        x = q % W;
        for (int j = 0; j < 3; ++j) { nx[j] = x - 1 + j; ny[j] = y - 1; }
    }
    const int g = y * W + x;
    // (-1 or not never changes in this kernel)
    if (__hip_atomic_load(&parent[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (nx[j] < 0 || nx[j] >= W || ny[j] < 0 || ny[j] >= H) continue;
        const int n = ny[j] * W + nx[j];
        if (__hip_atomic_load(&parent[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
        cc_union(parent, g, n);
    }
}

// launch 3 -----------------------------------------------------------------------------------------------------------------------------
// parent[] is only read here.  A pixel that is not its tile's local root still points at it (launch 2 moves roots only), a local root
// points at itself or at a smaller index anywhere: slot = the pointed-at pixel when that lies in this tile, else the pixel itself --
// either way a pixel of the same component inside the tile, and every final root is the slot of itself.
__global__ __launch_bounds__(CC_NT) void cc_stats_kernel(int H, int W, int ntx, void* scratch, int32_t* __restrict__ ids_out) {
    __shared__ int s_area[CC_PIX], s_r0[CC_PIX], s_r1[CC_PIX], s_c0[CC_PIX], s_c1[CC_PIX], s_root[CC_PIX];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / ntx) * CC_T, tx0 = (tile % ntx) * CC_T;
    const CcImage im = cc_image(scratch, b, H, W);
#pragma unroll
    for (int k = 0; k < CC_PIX / CC_NT; ++k) {
        const int li = threadIdx.x + k * CC_NT;
        s_area[li] = 0;
        s_r0[li] = INT_MAX;
        s_r1[li] = -1;
        s_c0[li] = INT_MAX;
        s_c1[li] = -1;
    }
    __syncthreads();
    // a thread owns four pixels side by side and adds a run of equal slots at once (one LDS atomic group per run, not per pixel)
    const int ly = threadIdx.x / (CC_T / 4), lx4 = (threadIdx.x % (CC_T / 4)) * 4;
    const int y = ty0 + ly;
    int slot[4];
    int run = -1, cnt = 0, xa = 0, xb = 0;
    auto flush = [&]() {
        if (run < 0) return;
        atomicAdd(&s_area[run], cnt);
        atomicMin(&s_r0[run], y);
        atomicMax(&s_r1[run], y);
        atomicMin(&s_c0[run], xa);
        atomicMax(&s_c1[run], xb);
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = tx0 + lx4 + j;
        slot[j] = -1;
        if (y < H && x < W) {
            const int g = y * W + x, p = im.parent[g];
            if (p >= 0) {
                const int py = p / W, px = p - py * W;
                const bool inside = py >= ty0 && py < ty0 + CC_T && px >= tx0 && px < tx0 + CC_T;
                slot[j] = inside ? (py - ty0) * CC_T + (px - tx0) : ly * CC_T + lx4 + j;
            }
        }
        if (slot[j] != run) {
            flush();
            run = slot[j];
            cnt = 0;
            xa = x;
        }
        cnt += 1;
        xb = x;
    }
    flush();
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_PIX / CC_NT; ++k) {
        const int li = threadIdx.x + k * CC_NT;
        const int a = s_area[li];
        if (a == 0) continue;
        const int g = (ty0 + li / CC_T) * W + tx0 + li % CC_T;
        const int r = cc_find(im.parent, g);
        s_root[li] = r;
        atomicAdd(&im.area[r], a);
        atomicMin(&im.r0[r], s_r0[li]);
        atomicMax(&im.r1[r], s_r1[li]);
        atomicMin(&im.c0[r], s_c0[li]);
        atomicMax(&im.c1[r], s_c1[li]);
        if (r == g) im.list[atomicAdd(&im.hdr[0], 1)] = g;          // at most cc_cap roots: the slot is inside the list
    }
    if (!ids_out) return;
    __syncthreads();
    int32_t* ids = ids_out + (size_t)b * H * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = tx0 + lx4 + j;
        if (y < H && x < W) ids[(size_t)y * W + x] = slot[j] < 0 ? -1 : s_root[slot[j]];
    }
}

// launch 4 -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long cc_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(CC_SEL_NT) void cc_select_kernel(int H, int W, int min_area, int max_out, void* scratch,
                                                             mkd_component* __restrict__ table, int32_t* __restrict__ count) {
    __shared__ int s_n;
    __shared__ unsigned long long s_part[2][CC_SEL_NT / 64];
    const int b = blockIdx.x;
    const CcImage im = cc_image(scratch, b, H, W);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int roots = im.hdr[0];
    for (int k = threadIdx.x; k < roots; k += CC_SEL_NT) {
        const int id = im.list[k], a = im.area[id];
        if (a >= min_area) im.keys[atomicAdd(&s_n, 1)] = ((unsigned long long)(unsigned)a << 32) | (unsigned)~id;
    }
    __syncthreads();          // (also makes the keys visible to the workgroup)
    const int n = s_n;
    if (threadIdx.x == 0) count[b] = n;
    unsigned long long prev = ~0ull;
    for (int r = 0; r < max_out; ++r) {
        unsigned long long best = 0;          // every key is > 0 (area >= 1) and unique (the id)
        for (int k = threadIdx.x; k < n; k += CC_SEL_NT) {
            const unsigned long long key = im.keys[k];
            if (key < prev && key > best) best = key;
        }
        best = cc_wave_max(best);
        if ((threadIdx.x & 63) == 0) s_part[r & 1][threadIdx.x >> 6] = best;
        __syncthreads();          // the other buffer is written next round, after everyone passed this barrier
        best = 0;
#pragma unroll
        for (int w = 0; w < CC_SEL_NT / 64; ++w) best = s_part[r & 1][w] > best ? s_part[r & 1][w] : best;
        if (threadIdx.x == 0) {
            mkd_component c = {-1, 0, INT_MAX, -1, INT_MAX, -1};
            if (best) {
                c.id = (int)~(unsigned)(best & 0xffffffffull);
                c.area = (int)(best >> 32);
                c.r0 = im.r0[c.id];
                c.r1 = im.r1[c.id];
                c.c0 = im.c0[c.id];
                c.c1 = im.c1[c.id];
            }
            table[(size_t)b * max_out + r] = c;
        }
        prev = best;          // 0 once the keys ran out: no key lies below it, the remaining rows are fill rows
    }
}

const char* cc_check(int batch, int H, int W) {
    if (batch < 1 || batch > 65535) return "batch must be 1..65535";
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 24)) return "H, W >= 1 and H * W <= 2^24";
    return nullptr;
}

// ---- owner map (mkd_owner_map): the nearest table component of every pixel ------------------------------------------------------------
// Exact Euclidean feature transform in two separable passes with a kernel boundary between them.  For pixel (y, x) and column u the
// nearest seed OF COLUMN u is g[y][u] rows away, so min over all seeds of (d^2, rank) = min over u of ((x - u)^2 + g[y][u]^2, the lowest
// rank among column u's seeds at that distance) -- at most two seeds of a column are g rows away (one up, one down), and a seed
// further than g from row y in its column never attains the minimum over its column.
//   1. om_column_kernel: a workgroup owns 64 consecutive columns (one per lane: every row access is coalesced) and OM_SEG row segments,
//      one wave each, so a column's sweeps are OM_SEG times shorter than its height.  Sweep down over the own segment: g = rows since
//      the segment's last seed; the segment's first and last seed go to LDS.  After the barrier, sweep up over what the first sweep
//      wrote (a seed is g == 0), starting from the first seed of the segments below and with the last seed of the segments above
//      standing in where the own segment had none yet: the nearer of the two, on a tie the lower rank.  The id -> rank lookup runs
//      over the image's table rows in LDS (up to the last row that holds an id), only where the id changes along the column.
//   2. om_row_kernel: one workgroup per (row, image) with the row's g and rank in LDS; a thread scans u = x, x -+ 1, x -+ 2, ... and keeps
//      the smallest key (d^2 << 8) | rank; it stops once off^2 alone exceeds the best d^2 (a column at an equal off^2 may still hold
//      the same d^2 with a lower rank, so equality goes on).  d^2 <= 2 * 2047^2 < 2^23: the key fits 31 bits.
constexpr int OM_MAX_SIDE = 2048;
constexpr int OM_COLS = 64;               // columns of a workgroup of the column pass: one per lane
constexpr int OM_SEG = 8;                 // row segments of a column: one wave each
constexpr int OM_COL_NT = OM_COLS * OM_SEG;
constexpr int OM_ROW_NT = 256;
constexpr int OM_CHUNK = 8;               // rows whose loads the column pass issues together
constexpr unsigned OM_NONE = 0xffffu;     // g: the column holds no seed (in that direction)
constexpr unsigned OM_NO_RANK = 255u;

__host__ __device__ inline size_t om_round256(size_t v) { return (v + 255) & ~(size_t)255; }

__global__ __launch_bounds__(OM_COL_NT) void om_column_kernel(const int32_t* __restrict__ ids, const mkd_component* __restrict__ table, int H, int W,
                                                              int max_out, uint16_t* __restrict__ g_out, uint8_t* __restrict__ rank_out) {
    __shared__ int s_id[CC_MAX_OUT];
    __shared__ int s_rows;                                 // 1 + the last table row that holds an id
    __shared__ int s_first[OM_SEG][OM_COLS], s_last[OM_SEG][OM_COLS];          // a segment's first / last seed: (y << 8) | rank, -1: none
    const int b = blockIdx.y;
    if (threadIdx.x < OM_COLS) {                           // (wave 0)
        const int id = (int)threadIdx.x < max_out ? table[(size_t)b * max_out + threadIdx.x].id : -1;
        s_id[threadIdx.x] = id;
        const unsigned long long held = __ballot(id >= 0);
        if (threadIdx.x == 0) s_rows = held ? 64 - __clzll((long long)held) : 0;
    }
    __syncthreads();
    const int rows = s_rows;
    const int lane = threadIdx.x & (OM_COLS - 1), seg = threadIdx.x / OM_COLS;
    const int x = blockIdx.x * OM_COLS + lane;
    const int per = (H + OM_SEG - 1) / OM_SEG;
    const int ya = min(seg * per, H), yb = min(ya + per, H);          // this thread's rows [ya, yb): empty past the image
    const bool active = x < W;
    const size_t base = (size_t)b * H * W + (active ? x : 0);
    const int32_t* idc = ids + base;
    uint16_t* gc = g_out + base;
    uint8_t* rc = rank_out + base;
    int first = -1, last = -1;
    if (active) {
        int last_id = -1;
        unsigned last_rank = OM_NO_RANK;                   // the rank of last_id
        for (int y0 = ya; y0 < yb; y0 += OM_CHUNK) {
            int v[OM_CHUNK];
#pragma unroll
            for (int k = 0; k < OM_CHUNK; ++k) v[k] = y0 + k < yb ? idc[(size_t)(y0 + k) * W] : -1;
#pragma unroll
            for (int k = 0; k < OM_CHUNK; ++k) {
                const int y = y0 + k;
                if (y >= yb) break;
                if (v[k] >= 0) {
                    if (v[k] != last_id) {
                        last_id = v[k];
                        last_rank = OM_NO_RANK;
                        for (int r = 0; r < rows; ++r)
                            if (s_id[r] == last_id) {      // the lowest row of a repeated id
                                last_rank = (unsigned)r;
                                break;
                            }
                    }
                    if (last_rank != OM_NO_RANK) {
                        last = (y << 8) | (int)last_rank;
                        if (first < 0) first = last;
                    }
                }
                gc[(size_t)y * W] = (uint16_t)(last < 0 ? OM_NONE : (unsigned)(y - (last >> 8)));
                rc[(size_t)y * W] = (uint8_t)(last < 0 ? OM_NO_RANK : (unsigned)(last & 255));
            }
        }
    }
    s_first[seg][lane] = first;
    s_last[seg][lane] = last;
    __syncthreads();
    if (!active) return;                                   // (after the last barrier)
    int above = -1, below = -1;                            // the nearest seed of the segments above / below this one
    for (int s = seg - 1; s >= 0 && above < 0; --s) above = s_last[s][lane];
    for (int s = seg + 1; s < OM_SEG && below < 0; ++s) below = s_first[s][lane];
    // up: a thread reads back its own stores only
    for (int y1 = yb - 1; y1 >= ya; y1 -= OM_CHUNK) {
        unsigned gd[OM_CHUNK], rd[OM_CHUNK];
#pragma unroll
        for (int k = 0; k < OM_CHUNK; ++k) {
            gd[k] = y1 - k >= ya ? gc[(size_t)(y1 - k) * W] : OM_NONE;
            rd[k] = y1 - k >= ya ? rc[(size_t)(y1 - k) * W] : OM_NO_RANK;
        }
#pragma unroll
        for (int k = 0; k < OM_CHUNK; ++k) {
            const int y = y1 - k;
            if (y < ya) break;
            if (gd[k] == 0u) {
                below = (y << 8) | (int)rd[k];
                continue;
            }
            unsigned g = gd[k], r = rd[k];
            if (g == OM_NONE && above >= 0) {              // no seed of the own segment above this row
                g = (unsigned)(y - (above >> 8));
                r = (unsigned)(above & 255);
            }
            if (below >= 0) {
                const unsigned du = (unsigned)((below >> 8) - y), ru = (unsigned)(below & 255);
                if (du < g || (du == g && ru < r)) {       // OM_NONE is larger than every distance
                    g = du;
                    r = ru;
                }
            }
            if (g != gd[k] || r != rd[k]) {
                gc[(size_t)y * W] = (uint16_t)g;
                rc[(size_t)y * W] = (uint8_t)r;
            }
        }
    }
}

__global__ __launch_bounds__(OM_ROW_NT) void om_row_kernel(const uint16_t* __restrict__ g_in, const uint8_t* __restrict__ rank_in, int H, int W,
                                                           uint8_t* __restrict__ owner, int32_t* __restrict__ dist2_out) {
    __shared__ uint16_t s_g[OM_MAX_SIDE];
    __shared__ uint8_t s_r[OM_MAX_SIDE];
    const size_t row = ((size_t)blockIdx.y * H + blockIdx.x) * W;
    for (int x = threadIdx.x; x < W; x += OM_ROW_NT) {
        s_g[x] = g_in[row + x];
        s_r[x] = rank_in[row + x];
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += OM_ROW_NT) {
        unsigned best = 0xffffffffu;                       // (best >> 8 = 2^24 - 1 exceeds every off^2 <= 2047^2)
        const int reach = max(x, W - 1 - x);
        for (int off = 0; off <= reach; ++off) {
            const unsigned o2 = (unsigned)(off * off);
            if (o2 > (best >> 8)) break;
            const int l = x - off, r = x + off;
            if (l >= 0) {
                const unsigned g = s_g[l];
                if (g != OM_NONE) best = min(best, ((o2 + g * g) << 8) | s_r[l]);
            }
            if (off > 0 && r < W) {
                const unsigned g = s_g[r];
                if (g != OM_NONE) best = min(best, ((o2 + g * g) << 8) | s_r[r]);
            }
        }
        const bool none = best == 0xffffffffu;
        owner[row + x] = (uint8_t)(none ? OM_NO_RANK : (best & 255u));
        if (dist2_out) dist2_out[row + x] = none ? INT_MAX : (int32_t)(best >> 8);
    }
}

const char* om_check(int batch, int H, int W) {
    if (batch < 1 || batch > 65535) return "batch must be 1..65535";
    if (H < 1 || W < 1 || H > OM_MAX_SIDE || W > OM_MAX_SIDE) return "H, W must be 1..2048";
    return nullptr;
}

// ---- owner weights (mkd_owner_weights): the window fraction of one (image, rank) per plane -----------------------------------------
// The three phases of paste_background_kernel (kernels_region.hip) on an indicator: the tile's owner == rank flags plus a halo of
// rho, clamped to the edge once, here (uint8 [(16 + 2 rho)][(64 + 2 rho)]); horizontal window sums (uint16 [(16 + 2 rho)][64]); 2 rho + 1
// rows of those per output pixel.  S <= 33^2: exact in fp32, one division.
constexpr int OW_TW = 64, OW_TH = 16, OW_MAX_FEATHER = 16;
struct OwArgs {
    int image[MKD_OWNER_MAX_ITEMS];
    int rank[MKD_OWNER_MAX_ITEMS];
};

__global__ __launch_bounds__(256) void owner_weights_kernel(const uint8_t* __restrict__ owner, const OwArgs a, int H, int W, int rho, int tiles_x,
                                                            float* __restrict__ w_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ow_smem[];
    const int i = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * OW_TH, x0 = tx * OW_TW;
    const int cw = OW_TW + 2 * rho, ch = OW_TH + 2 * rho, win = 2 * rho + 1;
    uint16_t* hs = (uint16_t*)ow_smem;                                       // [ch][64]
    uint8_t* flag = ow_smem + (size_t)ch * OW_TW * sizeof(uint16_t);         // [ch][cw]
    const uint8_t* ob = owner + (size_t)a.image[i] * H * W;
    const unsigned rank = (unsigned)a.rank[i];
    for (int e = threadIdx.x; e < ch * cw; e += 256) {
        const int ly = e / cw, lx = e - ly * cw;
        const int py = min(max(y0 - rho + ly, 0), H - 1), px = min(max(x0 - rho + lx, 0), W - 1);
        flag[e] = ob[(size_t)py * W + px] == rank ? 1 : 0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ch * OW_TW; e += 256) {
        const int ly = e >> 6, lx = e & 63;
        const uint8_t* row = flag + ly * cw + lx;
        unsigned s = 0;
        for (int d = 0; d < win; ++d) s += row[d];
        hs[e] = (uint16_t)s;
    }
    __syncthreads();
    const float D = (float)(win * win);
    for (int e = threadIdx.x; e < OW_TH * OW_TW; e += 256) {
        const int ly = e >> 6, lx = e & 63;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        unsigned s = 0;
        for (int d = 0; d < win; ++d) s += hs[(ly + d) * OW_TW + lx];
        w_out[((size_t)i * H + y) * W + x] = __fdiv_rn((float)s, D);
    }
}

}  // namespace

size_t mkd_owner_map_scratch_bytes(int batch, int H, int W) {
    if (const char* e = om_check(batch, H, W)) {
        mkd_set_error(std::string("mkd_owner_map_scratch_bytes: ") + e);
        return 0;
    }
    const size_t px = (size_t)batch * H * W;
    return om_round256(px * sizeof(uint16_t)) + om_round256(px);
}

int mkd_owner_map(const int32_t* ids, const mkd_component* table, int batch, int H, int W, int max_out, uint8_t* owner, int32_t* dist2_out,
                  void* scratch, void* stream) {
    const std::string who = "mkd_owner_map: ";
    if (const char* e = om_check(batch, H, W)) return mkd_fail(MKD_ERR_ARG, who + e);
    if (max_out < 1 || max_out > CC_MAX_OUT) return mkd_fail(MKD_ERR_ARG, who + "max_out must be 1..64");
    if (!ids || !table || !owner) return mkd_fail(MKD_ERR_ARG, who + "null ids / table / owner");
    if (!scratch || ((uintptr_t)scratch & 255)) return mkd_fail(MKD_ERR_ARG, who + "the scratch must be a 256-byte aligned device buffer");
    const hipStream_t st = (hipStream_t)stream;
    const size_t px = (size_t)batch * H * W;
    uint16_t* g = (uint16_t*)scratch;
    uint8_t* rk = (uint8_t*)scratch + om_round256(px * sizeof(uint16_t));
    hipLaunchKernelGGL(om_column_kernel, dim3((unsigned)((W + OM_COLS - 1) / OM_COLS), (unsigned)batch), dim3(OM_COL_NT), 0, st, ids, table, H, W,
                       max_out, g, rk);
    MKD_LAUNCH_CHECK("om_column_kernel");
    hipLaunchKernelGGL(om_row_kernel, dim3((unsigned)H, (unsigned)batch), dim3(OM_ROW_NT), 0, st, (const uint16_t*)g, (const uint8_t*)rk, H, W, owner,
                       dist2_out);
    MKD_LAUNCH_CHECK("om_row_kernel");
    return 0;
}

int mkd_owner_weights(const uint8_t* owner, int batch, int H, int W, const int32_t* items, int n, int feather, float* w_out, void* stream) {
    const std::string who = "mkd_owner_weights: ";
    if (const char* e = om_check(batch, H, W)) return mkd_fail(MKD_ERR_ARG, who + e);
    if (!owner || !items || !w_out) return mkd_fail(MKD_ERR_ARG, who + "null owner / items / w_out");
    if (n < 1 || n > MKD_OWNER_MAX_ITEMS) return mkd_fail(MKD_ERR_ARG, who + "1..16 items per call");
    if (feather < 0 || feather > OW_MAX_FEATHER) return mkd_fail(MKD_ERR_ARG, who + "feather must be 0..16");
    OwArgs a = {};
    for (int i = 0; i < n; ++i) {
        a.image[i] = items[2 * i];
        a.rank[i] = items[2 * i + 1];
        if (a.image[i] < 0 || a.image[i] >= batch) return mkd_fail(MKD_ERR_ARG, who + "an item's image lies outside the batch");
        if (a.rank[i] < 0 || a.rank[i] >= CC_MAX_OUT) return mkd_fail(MKD_ERR_ARG, who + "an item's rank must be 0..63");
    }
    const int tiles_x = (W + OW_TW - 1) / OW_TW, tiles_y = (H + OW_TH - 1) / OW_TH;          // <= 32 * 128 tiles
    const int ch = OW_TH + 2 * feather, cw = OW_TW + 2 * feather;
    const size_t lds = ((size_t)ch * OW_TW * sizeof(uint16_t) + (size_t)ch * cw + 15) & ~(size_t)15;          // <= 10752
    hipLaunchKernelGGL(owner_weights_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(256), lds, (hipStream_t)stream, owner, a, H, W,
                       feather, tiles_x, w_out);
    MKD_LAUNCH_CHECK("owner_weights_kernel");
    return 0;
}

size_t mkd_label_components_scratch_bytes(int batch, int H, int W) {
    if (const char* e = cc_check(batch, H, W)) {
        mkd_set_error(std::string("mkd_label_components_scratch_bytes: ") + e);
        return 0;
    }
    return (size_t)batch * cc_words(H, W) * sizeof(int32_t);
}

int mkd_label_components(const uint8_t* labels, int batch, int H, int W, uint64_t classes, int min_area, int max_out, mkd_component* table,
                         int32_t* count, int32_t* ids_out, void* scratch, void* stream) {
    const std::string who = "mkd_label_components: ";
    if (const char* e = cc_check(batch, H, W)) return mkd_fail(MKD_ERR_ARG, who + e);
    if (max_out < 1 || max_out > CC_MAX_OUT) return mkd_fail(MKD_ERR_ARG, who + "max_out must be 1..64");
    if (min_area < 1) return mkd_fail(MKD_ERR_ARG, who + "min_area must be >= 1");
    if (!labels || !table || !count) return mkd_fail(MKD_ERR_ARG, who + "null labels / table / count");
    if (!scratch || ((uintptr_t)scratch & 255)) return mkd_fail(MKD_ERR_ARG, who + "the scratch must be a 256-byte aligned device buffer");
    const hipStream_t st = (hipStream_t)stream;
    const int ntx = (W + CC_T - 1) / CC_T, nty = (H + CC_T - 1) / CC_T;
    const int nV = (ntx - 1) * H, nH = (nty - 1) * W;          // <= 2 * 2^24 / CC_T each
    const dim3 tiles((unsigned)(ntx * nty), (unsigned)batch);
    hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(CC_NT), 0, st, labels, H, W, ntx, classes, scratch);
    MKD_LAUNCH_CHECK("cc_tile_kernel");
    const int seam_blocks = (nV + nH + CC_NT - 1) / CC_NT;          // a single tile: one block whose threads all return
    hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)(seam_blocks < 1 ? 1 : seam_blocks), (unsigned)batch), dim3(CC_NT), 0, st, H, W, nV, nH,
                       scratch);
    MKD_LAUNCH_CHECK("cc_seam_kernel");
    hipLaunchKernelGGL(cc_stats_kernel, tiles, dim3(CC_NT), 0, st, H, W, ntx, scratch, ids_out);
    MKD_LAUNCH_CHECK("cc_stats_kernel");
    hipLaunchKernelGGL(cc_select_kernel, dim3((unsigned)batch), dim3(CC_SEL_NT), 0, st, H, W, min_area, max_out, scratch, table, count);
    MKD_LAUNCH_CHECK("cc_select_kernel");
    return 0;
}
