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

}  // namespace

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
