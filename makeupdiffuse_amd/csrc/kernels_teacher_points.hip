// Control points for the warped term of the teacher without landmarks (mkd_region_points, mkd_tps_solve; include/mkd.h holds the
// definitions, tests/teacher_points_ref.py restates them).  BUILD-DEFINED: the control points of a face are the centroid and the D
// support points of each of its four exclusive regions (pgt_regions.h), and the thin-plate spline through the pairs (source point ->
// reference point) is solved on the device, so the warped teacher needs no file and no host round trip.
//
// Points: three launches.  Clear; accumulate -- 256 threads x 4 consecutive pixels, a thread folds its run of one region in registers,
// the workgroup folds in LDS (64-bit add for the moments, 64-bit max for the support keys), then one global atomic per touched cell;
// finish -- a thread per (image, region) turns the cells into points.  Everything is integer but the two divisions of a centroid, so
// the bytes do not depend on the order of the atomics.
//
// Solve: one launch, one workgroup of 256 threads per sample, the augmented (k + 3) x (k + 5) system in dynamic LDS.  Gaussian
// elimination with partial pivoting: every wave finds the pivot of a column on its own (the same values, the same answer, nothing to broadcast),
// four threads share a row of the update.  No atomics and a fixed order of every sum: the bytes repeat from run to run.  NOTHING
// CONTRACTS (build.py compiles this file with -ffp-contract=off, as it does kernels_teacher_warp.hip).
#include "mkd_common.h"
#include "pgt_regions.h"
#include "../../include/mkd.h"

#include <math.h>

namespace {

// ---- mkd_region_points ---------------------------------------------------------------------------------------------------------------
constexpr int RP_NT = 256;                      // threads of the accumulate kernel
constexpr int RP_PER = 4;                       // consecutive pixels per thread
constexpr int RP_MAXD = 16;
constexpr int RP_CELLS = 3 + RP_MAXD;           // per (image, region): n, sum y, sum x, then the key of each direction
constexpr int RP_IMG = 4 * RP_CELLS;            // cells of one image

// (cq, sq) of direction d of 16, y pointing down: 16384 (cos, sin)(d * 22.5 deg) rounded; D = 8 takes every second one
__constant__ int rp_dir[RP_MAXD][2] = {{16384, 0},  {15137, 6270},   {11585, 11585},   {6270, 15137},   {0, 16384},  {-6270, 15137},  {-11585, 11585},  {-15137, 6270},
                                       {-16384, 0}, {-15137, -6270}, {-11585, -11585}, {-6270, -15137}, {0, -16384}, {6270, -15137},  {11585, -11585},  {15137, -6270}};

// larger projection first, then the smaller linear index; 0 is "no pixel" (no pixel has it: the low word of a key is >= 2^32 - 2^24)
__device__ __forceinline__ unsigned long long rp_key(int proj, unsigned lin) {
    return ((unsigned long long)((unsigned)proj + 0x80000000u) << 32) | (unsigned long long)(0xFFFFFFFFu - lin);
}

__global__ __launch_bounds__(RP_NT) void rp_clear_kernel(unsigned long long* __restrict__ cells, int ncells) {
    const int k = blockIdx.x * RP_NT + threadIdx.x;
    if (k < ncells) cells[k] = 0ull;
}

// grid (ceil(H W / 1024), n); D is a template argument so that the keys of a run stay in registers
template <int D>
__global__ __launch_bounds__(RP_NT) void rp_accumulate_kernel(const uint8_t* __restrict__ masks, int n, int H, int W,
                                                              unsigned long long* __restrict__ cells) {
    __shared__ unsigned long long s_cell[RP_IMG];
    constexpr int step = RP_MAXD / D;
    const int b = blockIdx.y;
    for (int k = threadIdx.x; k < RP_IMG; k += RP_NT) s_cell[k] = 0ull;
    __syncthreads();
    const unsigned npix = (unsigned)H * (unsigned)W;          // <= 2^24
    const size_t plane = (size_t)n * npix;
    const uint8_t* mk = masks + (size_t)b * npix;
    const unsigned p0 = (blockIdx.x * RP_NT + threadIdx.x) * RP_PER;
    // a thread's run of pixels of one region is folded in registers and goes to LDS once
    int run = 0;
    unsigned long long cnt = 0, sy = 0, sx = 0, key[D];
    auto flush = [&]() {
        if (run == 0) return;
        unsigned long long* c = s_cell + (run - 1) * RP_CELLS;
        atomicAdd(c, cnt);
        atomicAdd(c + 1, sy);
        atomicAdd(c + 2, sx);
#pragma unroll
        for (int d = 0; d < D; ++d)
            // The plain read races with the other threads' atomics on the cell, harmlessly: an aligned 64-bit LDS read is one untorn
            // access, a cell only grows, so a stale value is never above the cell and costs at most one atomic that changes nothing.
            if (key[d] > c[3 + d]) atomicMax(c + 3 + d, key[d]);
    };
    if (p0 < npix) {
        unsigned y = p0 / (unsigned)W, x = p0 - y * (unsigned)W;
        for (int k = 0; k < RP_PER && p0 + k < npix; ++k) {
            const size_t p = p0 + k;
            const int id = pg_id(mk[p], mk[plane + p], mk[2 * plane + p], mk[3 * plane + p]);
            if (id != run) {
                flush();
                run = id;
                cnt = sy = sx = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) key[d] = 0ull;
            }
            if (id) {
                ++cnt;
                sy += y;
                sx += x;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const unsigned long long kd = rp_key(rp_dir[d * step][0] * (int)x + rp_dir[d * step][1] * (int)y, (unsigned)p);      // |proj| < 2^27
                    key[d] = kd > key[d] ? kd : key[d];
                }
            }
            if (++x == (unsigned)W) {
                x = 0;
                ++y;
            }
        }
        flush();
    }
    __syncthreads();
    unsigned long long* g = cells + (size_t)b * RP_IMG;
    for (int k = threadIdx.x; k < RP_IMG; k += RP_NT) {
        const unsigned long long v = s_cell[k];
        if (v == 0ull) continue;
        if (k % RP_CELLS < 3)
            atomicAdd(g + k, v);
        else
            atomicMax(g + k, v);
    }
}

// one thread per (image, region id r = 1..4)
__global__ __launch_bounds__(RP_NT) void rp_finish_kernel(const unsigned long long* __restrict__ cells, int n, int W, int D, int min_area,
                                                          double* __restrict__ pts, int32_t* __restrict__ use, int32_t* __restrict__ count) {
    const int t = blockIdx.x * RP_NT + threadIdx.x;
    if (t >= n * 4) return;
    const unsigned long long* c = cells + (size_t)t * RP_CELLS;
    const long long nr = (long long)c[0];
    const bool on = nr >= (long long)min_area;
    const size_t o = (size_t)t * (D + 1);          // = (image * 4 + (r - 1)) * (D + 1): K = 4 (D + 1) points per image
    if (count) count[t] = (int32_t)nr;
    pts[2 * o] = on ? (double)(long long)c[1] / (double)nr : 0.0;
    pts[2 * o + 1] = on ? (double)(long long)c[2] / (double)nr : 0.0;
    use[o] = on ? 1 : 0;
    for (int d = 0; d < D; ++d) {
        const unsigned lin = 0xFFFFFFFFu - (unsigned)(c[3 + d] & 0xFFFFFFFFull);
        const unsigned y = lin / (unsigned)W;
        pts[2 * (o + 1 + d)] = on ? (double)y : 0.0;
        pts[2 * (o + 1 + d) + 1] = on ? (double)(lin - y * (unsigned)W) : 0.0;
        use[o + 1 + d] = on ? 1 : 0;
    }
}

size_t rp_scratch(int n) { return ((size_t)n * RP_IMG * sizeof(unsigned long long) + 255) & ~(size_t)255; }

// ---- mkd_tps_solve -------------------------------------------------------------------------------------------------------------------
constexpr int TS_NT = 256;
constexpr int TS_MAXK = 128;
constexpr double TS_RESIDUAL = 1e-6;          // teacher.TPS_RESIDUAL

struct TsPair { double y, x; };

__device__ __forceinline__ bool ts_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for a NaN

// the augmented system [[U(|c_i - c_j|^2), P | d], [P^T, 0 | 0]], P = [1, y, x], into A (N = k + 3 rows of stride ld, N + 2 columns)
__device__ __forceinline__ void ts_fill(double* A, int ld, const TsPair* c, const TsPair* d, int k) {
    const int N = k + 3, cols = N + 2;
    for (int e = threadIdx.x; e < N * cols; e += TS_NT) {
        const int i = e / cols, j = e - i * cols;
        double v = 0.0;
        if (i < k && j < k) {
            const double dy = c[i].y - c[j].y, dx = c[i].x - c[j].x;
            const double s = dy * dy + dx * dx;
            v = s > 0.0 ? s * log(s) : 0.0;
        } else if (i < k) {
            v = j == k ? 1.0 : j == k + 1 ? c[i].y : j == k + 2 ? c[i].x : j == N ? d[i].y : d[i].x;
        } else if (j < k) {
            v = i == k ? 1.0 : i == k + 1 ? c[j].y : c[j].x;
        }
        A[i * ld + j] = v;
    }
}

// grid (B), 256 threads, (max_ctrl + 3) (max_ctrl + 5) doubles of dynamic LDS
__global__ __launch_bounds__(TS_NT) void tps_solve_kernel(const double* __restrict__ pts_src, const double* __restrict__ pts_ref,
                                                          const int32_t* __restrict__ use_src, const int32_t* __restrict__ use_ref, int K, int M,
                                                          double* __restrict__ ctrl, double* __restrict__ coef, int32_t* __restrict__ kcount) {
    extern __shared__ __attribute__((aligned(16))) double A[];
    __shared__ TsPair s_c[TS_MAXK], s_d[TS_MAXK];          // the kept pairs: control point, target
    __shared__ TsPair s_sol[TS_MAXK + 3];
    __shared__ int s_keep[TS_MAXK];
    const int tid = threadIdx.x, b = blockIdx.x, ld = M + 5;
    const double* ps = pts_src + (size_t)b * K * 2;
    const double* pr = pts_ref + (size_t)b * K * 2;

    // 1, 2: the pairs in use, minus those whose source point repeats an earlier one of them
    bool used = false, bad = false;
    TsPair c = {0.0, 0.0}, d = {0.0, 0.0};
    if (tid < K) {
        used = (!use_src || use_src[(size_t)b * K + tid] != 0) && (!use_ref || use_ref[(size_t)b * K + tid] != 0);
        if (used) {
            c = {ps[2 * tid], ps[2 * tid + 1]};
            d = {pr[2 * tid], pr[2 * tid + 1]};
            bad = !(ts_finite(c.y) && ts_finite(c.x) && ts_finite(d.y) && ts_finite(d.x));
        }
        s_keep[tid] = used;
        s_sol[tid] = c;          // (staging: the source point of every pair)
    }
    bool fail = __syncthreads_or(bad) != 0;
    // "Equals an earlier KEPT pair" is tested as "equals an earlier pair IN USE": == is transitive on finite values, so the first pair of
    // every run of equal source points is kept and every later one equals it; a sample with a non-finite value has failed already.
    bool keep = used;
    if (used)
        for (int j = 0; j < tid; ++j)
            if (s_keep[j] && s_sol[j].y == c.y && s_sol[j].x == c.x) keep = false;
    __syncthreads();
    if (tid < K) s_keep[tid] = keep;
    __syncthreads();
    int k = 0, at = 0;
    for (int j = 0; j < K; ++j) {
        at += j < tid ? s_keep[j] : 0;
        k += s_keep[j];
    }
    if (keep) {
        s_c[at] = c;
        s_d[at] = d;
    }
    fail = fail || k < 3;
    const int N = k + 3;
    __syncthreads();

    if (!fail) {
        // 3, 4: eliminate column p below the pivot, the right sides along
        ts_fill(A, ld, s_c, s_d, k);
        __syncthreads();
        for (int p = 0; p < N; ++p) {
            // every wave on its own: the row of the largest |A[i][p]|, i >= p, ties to the lowest row; not finite counts as infinite
            double best = -1.0;
            int row = N;
            for (int i = p + (tid & 63); i < N; i += 64) {
                double m = fabs(A[i * ld + p]);
                m = ts_finite(m) ? m : INFINITY;
                if (m > best) {
                    best = m;
                    row = i;
                }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double ob = __shfl_xor(best, o);
                const int orow = __shfl_xor(row, o);
                if (ob > best || (ob == best && orow < row)) {
                    best = ob;
                    row = orow;
                }
            }
            if (best == 0.0 || !ts_finite(best)) {          // (the same in every wave)
                fail = true;
                break;
            }
            __syncthreads();          // (every wave has read column p before a swap moves it)
            if (row != p)
                for (int j = p + tid; j < N + 2; j += TS_NT) {
                    const double u = A[p * ld + j];
                    A[p * ld + j] = A[row * ld + j];
                    A[row * ld + j] = u;
                }
            __syncthreads();
            const double piv = A[p * ld + p];
            for (int i = p + 1 + (tid >> 2); i < N; i += TS_NT / 4) {
                const double f = A[i * ld + p] / piv;          // (column p itself is left as it is: nobody reads it again)
                for (int j = p + 1 + (tid & 3); j < N + 2; j += 4) A[i * ld + j] = A[i * ld + j] - f * A[p * ld + j];
            }
            __syncthreads();
        }
    }
    if (!fail) {
        // back substitution, column-oriented: x_p, then every row above gives up its term of x_p (p = N - 1 .. 0: a fixed order per row)
        for (int p = N - 1; p >= 0; --p) {
            if (tid < 2) {
                const double v = A[p * ld + N + tid] / A[p * ld + p];
                if (tid == 0) s_sol[p].y = v; else s_sol[p].x = v;
            }
            __syncthreads();
            const TsPair xp = s_sol[p];
            for (int e = tid; e < 2 * p; e += TS_NT) {
                const int i = e >> 1;
                A[i * ld + N + (e & 1)] = A[i * ld + N + (e & 1)] - A[i * ld + p] * ((e & 1) ? xp.x : xp.y);
            }
            __syncthreads();
        }
        // 5: the system again, and what the solution leaves of every row of it
        ts_fill(A, ld, s_c, s_d, k);
        __syncthreads();
        bool off = false;
        for (int e = tid; e < 2 * N; e += TS_NT) {
            const int i = e >> 1, col = e & 1;
            double acc = 0.0;
            for (int j = 0; j < N; ++j) acc = acc + A[i * ld + j] * (col ? s_sol[j].x : s_sol[j].y);
            const double sol = col ? s_sol[i].x : s_sol[i].y;
            off = off || !ts_finite(sol) || !(fabs(acc - A[i * ld + N + col]) <= TS_RESIDUAL);
        }
        fail = __syncthreads_or(off) != 0;
    }

    // 6: the layout mkd_pgt_warp reads; unused slots and a dropped sample are zeros
    const int kb = fail ? 0 : k;
    double* cb = ctrl + (size_t)b * M * 2;
    double* fb = coef + (size_t)b * 2 * (M + 3);
    for (int e = tid; e < 2 * M; e += TS_NT) {
        const int i = e >> 1;
        cb[e] = i < kb ? ((e & 1) ? s_c[i].x : s_c[i].y) : 0.0;
    }
    for (int e = tid; e < 2 * (M + 3); e += TS_NT) {
        const int col = e / (M + 3), j = e - col * (M + 3);
        const int from = j < M ? (j < kb ? j : -1) : kb + (j - M);
        fb[e] = kb && from >= 0 ? (col ? s_sol[from].x : s_sol[from].y) : 0.0;
    }
    if (tid == 0) kcount[b] = kb;
}

inline bool tp_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

size_t mkd_region_points_scratch_bytes(int n) {
    if (n < 1 || n > 65535) {
        mkd_set_error("mkd_region_points_scratch_bytes: n must be 1..65535");
        return 0;
    }
    return rp_scratch(n);
}

int mkd_region_points_launches(void) { return 3; }

int mkd_region_points(const uint8_t* masks, int n, int H, int W, int dirs, int min_area, double* pts, int32_t* use, int32_t* count,
                      void* scratch, void* stream) {
    const std::string who = "mkd_region_points: ";
    if (n < 1 || n > 65535) return mkd_fail(MKD_ERR_ARG, who + "n must be 1..65535");
    if (H < 1 || W < 1 || H > 4096 || W > 4096 || (int64_t)H * W > (1 << 24)) return mkd_fail(MKD_ERR_ARG, who + "H, W must be 1..4096 with H * W <= 2^24");
    if (dirs != 8 && dirs != 16) return mkd_fail(MKD_ERR_ARG, who + "dirs must be 8 or 16");
    if (min_area < 1) return mkd_fail(MKD_ERR_ARG, who + "min_area must be >= 1");
    if (!masks || !pts || !use) return mkd_fail(MKD_ERR_ARG, who + "null masks / pts / use");
    if (!tp_aligned(pts, 8) || !tp_aligned(use, 4) || !tp_aligned(count, 4)) return mkd_fail(MKD_ERR_ARG, who + "pts must be 8-byte, use / count 4-byte aligned");
    if (!scratch || !tp_aligned(scratch, 256)) return mkd_fail(MKD_ERR_ARG, who + "the scratch must be a 256-byte aligned device buffer");
    const hipStream_t st = (hipStream_t)stream;
    unsigned long long* cells = (unsigned long long*)scratch;
    const int ncells = n * RP_IMG;          // < 2^23
    const dim3 pix((unsigned)(((size_t)H * W + (size_t)RP_NT * RP_PER - 1) / ((size_t)RP_NT * RP_PER)), (unsigned)n);      // x <= 16384
    hipLaunchKernelGGL(rp_clear_kernel, dim3((unsigned)((ncells + RP_NT - 1) / RP_NT)), dim3(RP_NT), 0, st, cells, ncells);
    MKD_LAUNCH_CHECK("rp_clear_kernel");
    if (dirs == 8)
        hipLaunchKernelGGL(rp_accumulate_kernel<8>, pix, dim3(RP_NT), 0, st, masks, n, H, W, cells);
    else
        hipLaunchKernelGGL(rp_accumulate_kernel<16>, pix, dim3(RP_NT), 0, st, masks, n, H, W, cells);
    MKD_LAUNCH_CHECK("rp_accumulate_kernel");
    hipLaunchKernelGGL(rp_finish_kernel, dim3((unsigned)((n * 4 + RP_NT - 1) / RP_NT)), dim3(RP_NT), 0, st, (const unsigned long long*)cells, n, W, dirs,
                       min_area, pts, use, count);
    MKD_LAUNCH_CHECK("rp_finish_kernel");
    return 0;
}

int mkd_tps_solve_launches(void) { return 1; }

int mkd_tps_solve(const double* pts_src, const double* pts_ref, const int32_t* use_src, const int32_t* use_ref, int B, int K, int max_ctrl,
                  double* ctrl, double* coef, int32_t* kcount, void* stream) {
    const std::string who = "mkd_tps_solve: ";
    if (B < 1 || B > 65535) return mkd_fail(MKD_ERR_ARG, who + "B must be 1..65535");
    if (K < 1 || K > max_ctrl || max_ctrl > TS_MAXK) return mkd_fail(MKD_ERR_ARG, who + "1 <= K <= max_ctrl <= 128");
    if (!pts_src || !pts_ref || !ctrl || !coef || !kcount) return mkd_fail(MKD_ERR_ARG, who + "null pts_src / pts_ref / ctrl / coef / kcount");
    if (!tp_aligned(pts_src, 8) || !tp_aligned(pts_ref, 8) || !tp_aligned(ctrl, 8) || !tp_aligned(coef, 8) || !tp_aligned(kcount, 8))
        return mkd_fail(MKD_ERR_ARG, who + "pts_src / pts_ref / ctrl / coef / kcount must be 8-byte aligned");
    if (!tp_aligned(use_src, 4) || !tp_aligned(use_ref, 4)) return mkd_fail(MKD_ERR_ARG, who + "use_src / use_ref must be 4-byte aligned");
    const size_t lds = (size_t)(max_ctrl + 3) * (max_ctrl + 5) * sizeof(double);          // 139,384 bytes at 128: one workgroup per CU
    if (lds > 64 * 1024) {          // on every such call: the limit belongs to the function on the CURRENT device, and setting it is a cheap host call
        const hipError_t e = hipFuncSetAttribute((const void*)tps_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)((TS_MAXK + 3) * (TS_MAXK + 5) * sizeof(double)));
        if (e != hipSuccess) return mkd_fail(-2, who + "hipFuncSetAttribute(max dynamic LDS): " + hipGetErrorString(e));
    }
    hipLaunchKernelGGL(tps_solve_kernel, dim3((unsigned)B), dim3(TS_NT), lds, (hipStream_t)stream, pts_src, pts_ref, use_src, use_ref, K, max_ctrl, ctrl,
                       coef, kcount);
    MKD_LAUNCH_CHECK("tps_solve_kernel");
    return 0;
}

}  // extern "C"
