// Region-wise histogram matching and its L1 score (reference diffmk/histogram_matching.py:41-66 through diffmk/makeups.py:232-245
// criterionHis), and the region masks of diffmk/makeups.py:179-230, batched over n independent terms.  Every result that the
// reference defines is an integer (counts, tables, matched values) and is reproduced exactly; the loss is a fixed-order sum.
//
// One term = (dst image, ref image, dst mask, ref mask), images fp32 [3, H, W] in [0, 1]:
//   v = clamp(x, 0, 1) * 255 (fp32, one rounding); 256-bin counts of v under each mask; pdf = count / total (IEEE fp32 division);
//   cdf by SEQUENTIAL fp32 adds; table[i] = first j in 1..255 with cdf_ref[j-1] <= cdf_dst[i] <= cdf_ref[j], else i
//   (table[0] = 0, table[255] = 255); matched = table[int(v)] under the dst mask, 0 elsewhere; loss = mean |v mask - matched|.
// A scoring call is at most five launches whatever n: zero the counters, histogram, CDF + table, apply + partial sums, final sum.
#include "mkd_common.h"
#include <climits>

namespace {

constexpr int HM_WGS = 64;                 // workgroups per (term, side): fixed, so a term's partial sums do not depend on n
constexpr int HM_REPL = 8;                 // LDS replicas of the 3 x 256 counters, picked by lane & 7
constexpr int HM_RSTRIDE = 3 * 256 + 8;    // replica stride in words: shifts a bin by 8 banks per replica (768 % 64 == 0 would stack them)
constexpr int RM_WGS = 16;                 // workgroups per label map of the region-mask kernels

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- region masks --------------------------------------------------------------------------------------------------------------
__global__ void region_init_kernel(int32_t* __restrict__ count, int32_t* __restrict__ box, int batch) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    count[i] = 0;
    if (box) { box[4 * i] = INT_MAX; box[4 * i + 1] = -1; box[4 * i + 2] = INT_MAX; box[4 * i + 3] = -1; }
}

// bounding box (row min, row max, col min, col max) of the pixels whose label is in box_classes: wave reduce, one atomic pair per wave
__global__ __launch_bounds__(256) void region_box_kernel(const uint8_t* __restrict__ labels, int H, int W, unsigned long long box_classes,
                                                         int32_t* __restrict__ box) {
    const int b = blockIdx.y, HW = H * W;
    const uint8_t* lab = labels + (size_t)b * HW;
    int r0 = INT_MAX, r1 = -1, c0 = INT_MAX, c1 = -1;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
        const unsigned l = lab[p];
        if (l < 64u && ((box_classes >> l) & 1ull)) {
            const int y = p / W, x = p - y * W;
            r0 = min(r0, y); r1 = max(r1, y); c0 = min(c0, x); c1 = max(c1, x);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        r0 = min(r0, __shfl_xor(r0, o, 64)); r1 = max(r1, __shfl_xor(r1, o, 64));
        c0 = min(c0, __shfl_xor(c0, o, 64)); c1 = max(c1, __shfl_xor(c1, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && r1 >= 0) {
        atomicMin(&box[4 * b], r0); atomicMax(&box[4 * b + 1], r1);
        atomicMin(&box[4 * b + 2], c0); atomicMax(&box[4 * b + 3], c1);
    }
}

// mask = label in classes [and inside the box grown by margin, clipped to the image]; count = its pixels
__global__ __launch_bounds__(256) void region_mask_kernel(const uint8_t* __restrict__ labels, int H, int W, unsigned long long classes,
                                                          int use_box, int margin, const int32_t* __restrict__ box,
                                                          uint8_t* __restrict__ mask, int32_t* __restrict__ count) {
    const int b = blockIdx.y, HW = H * W;
    const uint8_t* lab = labels + (size_t)b * HW;
    uint8_t* out = mask + (size_t)b * HW;
    int r0 = 0, r1 = H - 1, c0 = 0, c1 = W - 1;
    if (use_box) {
        const int br0 = box[4 * b], br1 = box[4 * b + 1], bc0 = box[4 * b + 2], bc1 = box[4 * b + 3];
        if (br1 < 0) { r0 = 1; r1 = 0; }          // no pixel of box_classes: an empty region
        else { r0 = max(br0 - margin, 0); r1 = min(br1 + margin, H - 1); c0 = max(bc0 - margin, 0); c1 = min(bc1 + margin, W - 1); }
    }
    int cnt = 0;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
        const unsigned l = lab[p];
        const int y = p / W, x = p - y * W;
        const int in = (l < 64u && ((classes >> l) & 1ull) && y >= r0 && y <= r1 && x >= c0 && x <= c1) ? 1 : 0;
        out[p] = (uint8_t)in;
        cnt += in;
    }
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&count[b], cnt);
}

// ---- masked histogram ----------------------------------------------------------------------------------------------------------
// grid (HM_WGS, n, 2): side 0 = dst under mask_dst, side 1 = ref under mask_ref.  index [n][4] = (dst image, ref image, dst mask,
// ref mask) of term t, null: t for all four.  vec: HW % 4 == 0 and 16-byte aligned bases (4 pixels per lane, 16-byte loads).
__global__ __launch_bounds__(256) void hist_kernel(const float* __restrict__ dst, const float* __restrict__ ref, const uint8_t* __restrict__ mdst,
                                                   const uint8_t* __restrict__ mref, const int32_t* __restrict__ index, int HW, int vec,
                                                   uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[HM_REPL * HM_RSTRIDE];
    const int t = blockIdx.y, side = blockIdx.z;
    for (int i = threadIdx.x; i < HM_REPL * HM_RSTRIDE; i += 256) lh[i] = 0u;
    __syncthreads();
    const int ii = index ? index[4 * t + side] : t, im = index ? index[4 * t + 2 + side] : t;
    const float* img = (side ? ref : dst) + (size_t)ii * 3 * HW;
    const uint8_t* m = (side ? mref : mdst) + (size_t)im * HW;
    uint32_t* my = lh + (threadIdx.x & (HM_REPL - 1)) * HM_RSTRIDE;
    const int ngroups = (HW + 3) >> 2;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
        const int p = g * 4;
        if (vec) {
            const uint32_t mm = *(const uint32_t*)(m + p);
            if (!mm) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 v = *(const f32x4*)(img + (size_t)c * HW + p);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if ((mm >> (8 * k)) & 0xffu) atomicAdd(&my[c * 256 + hm_bin(hm_value(v[k]))], 1u);
            }
        } else {
            for (int k = 0; k < 4 && p + k < HW; ++k) {
                if (!m[p + k]) continue;
                for (int c = 0; c < 3; ++c) atomicAdd(&my[c * 256 + hm_bin(hm_value(img[(size_t)c * HW + p + k]))], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* out = hist + (size_t)(t * 2 + side) * 3 * 256;
    for (int i = threadIdx.x; i < 3 * 256; i += 256) {
        uint32_t s = 0;
#pragma unroll
        for (int r = 0; r < HM_REPL; ++r) s += lh[r * HM_RSTRIDE + i];
        if (s) atomicAdd(&out[i], s);
    }
}

// ---- CDF + table: one 256-thread workgroup per (channel, term) --------------------------------------------------------------------
// The divisions are element-wise (thread i), the CDF is ONE lane's chain of 255 correctly rounded adds per side (the table compares
// these floats with <= / >=, so neither a parallel scan nor a contracted form may replace it); thread i then searches its entry.
__global__ __launch_bounds__(256) void table_kernel(const uint32_t* __restrict__ hist, uint8_t* __restrict__ tab_s, uint8_t* __restrict__ tab_user,
                                                    int32_t* __restrict__ cnt_s, int32_t* __restrict__ cnt_user) {
    __shared__ float cd[256], cr[256];
    __shared__ int tot[2][4];
    const int c = blockIdx.x, t = blockIdx.y, i = threadIdx.x;
    const uint32_t hd = hist[((size_t)(t * 2 + 0) * 3 + c) * 256 + i], hr = hist[((size_t)(t * 2 + 1) * 3 + c) * 256 + i];
    const int sd = wave_sum_i((int)hd), sr = wave_sum_i((int)hr);
    if ((i & 63) == 0) { tot[0][i >> 6] = sd; tot[1][i >> 6] = sr; }
    __syncthreads();
    const int totd = tot[0][0] + tot[0][1] + tot[0][2] + tot[0][3], totr = tot[1][0] + tot[1][1] + tot[1][2] + tot[1][3];
    int entry = i;
    if (totd > 0 && totr > 0) {            // block-uniform.  An empty side: the identity table (build-defined)
        cd[i] = __fdiv_rn((float)hd, (float)totd);
        cr[i] = __fdiv_rn((float)hr, (float)totr);
        __syncthreads();
        if (i == 0 || i == 64) {           // two waves, one chain each
            float* a = i ? cr : cd;
            float s = a[0];
            for (int k = 1; k < 256; ++k) { s = __fadd_rn(s, a[k]); a[k] = s; }
        }
        __syncthreads();
        if (i >= 1 && i <= 254) {
            const float x = cd[i];
            for (int j = 1; j < 256; ++j)
                if (x >= cr[j - 1] && x <= cr[j]) { entry = j; break; }
        }
    }
    tab_s[((size_t)t * 3 + c) * 256 + i] = (uint8_t)entry;
    if (tab_user) tab_user[((size_t)t * 3 + c) * 256 + i] = (uint8_t)entry;
    if (c == 0 && i < 2) {
        const int v = i ? totr : totd;
        cnt_s[2 * t + i] = v;
        if (cnt_user) cnt_user[2 * t + i] = v;
    }
}

// ---- apply + L1 ----------------------------------------------------------------------------------------------------------------
// grid (HM_WGS, n).  matched (may be null) [n, 3, HW] in 0..255; partial (may be null) [n][HM_WGS] fp64: this workgroup's sum of
// |v mask - matched| in a fixed order (per-lane fp64 accumulation, xor-shuffle tree, four wave sums added in order): bit-repeatable,
// and the 16-byte and the scalar-load form give a lane the same pixels in the same order, so the bits do not depend on alignment.
__global__ __launch_bounds__(256) void apply_kernel(const float* __restrict__ dst, const uint8_t* __restrict__ mdst, const int32_t* __restrict__ index,
                                                    int HW, int vec, const uint8_t* __restrict__ tab_s, const int32_t* __restrict__ cnt_s,
                                                    float* __restrict__ matched, double* __restrict__ partial) {
    __shared__ uint8_t tab[3 * 256];
    __shared__ double wsum[4];
    const int t = blockIdx.y;
    for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = tab_s[(size_t)t * 3 * 256 + i];
    __syncthreads();
    const bool live = cnt_s[2 * t] > 0 && cnt_s[2 * t + 1] > 0;        // an empty side: matched = 0, loss 0
    const int ii = index ? index[4 * t] : t, im = index ? index[4 * t + 2] : t;
    const float* img = dst + (size_t)ii * 3 * HW;
    const uint8_t* m = mdst + (size_t)im * HW;
    float* out = matched ? matched + (size_t)t * 3 * HW : nullptr;
    double acc = 0.0;
    const int ngroups = (HW + 3) >> 2;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
        const int p = g * 4;
        if (vec) {
            const uint32_t mm = live ? *(const uint32_t*)(m + p) : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (mm) {
                    const f32x4 x = *(const f32x4*)(img + (size_t)c * HW + p);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if ((mm >> (8 * k)) & 0xffu) {
                            const float v = hm_value(x[k]);
                            o[k] = (float)tab[c * 256 + hm_bin(v)];
                            acc += (double)fabsf(__fsub_rn(v, o[k]));
                        }
                }
                if (out) *(f32x4*)(out + (size_t)c * HW + p) = o;
            }
        } else {
            for (int c = 0; c < 3; ++c)              // channel-major like the 16-byte form: a lane adds its terms in the same order
                for (int k = 0; k < 4 && p + k < HW; ++k) {
                    float o = 0.f;
                    if (live && m[p + k]) {
                        const float v = hm_value(img[(size_t)c * HW + p + k]);
                        o = (float)tab[c * 256 + hm_bin(v)];
                        acc += (double)fabsf(__fsub_rn(v, o));
                    }
                    if (out) out[(size_t)c * HW + p + k] = o;
                }
        }
    }
    if (!partial) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)t * HM_WGS + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ void loss_kernel(const double* __restrict__ partial, int n, double count, float* __restrict__ loss) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    double s = 0.0;
    for (int k = 0; k < HM_WGS; ++k) s += partial[(size_t)t * HM_WGS + k];
    loss[t] = (float)(s / count);
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
struct HmScratch { size_t hist, tab, cnt, part, total; };
inline HmScratch hm_layout(int n) {
    HmScratch s;
    s.hist = 0;
    s.tab = up256((size_t)n * 2 * 3 * 256 * sizeof(uint32_t));
    s.cnt = s.tab + up256((size_t)n * 3 * 256);
    s.part = s.cnt + up256((size_t)n * 2 * sizeof(int32_t));
    s.total = s.part + up256((size_t)n * HM_WGS * sizeof(double));
    return s;
}
inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

int launch_region_mask_from_labels(const uint8_t* labels, int batch, int H, int W, uint64_t classes, uint64_t box_classes, int margin,
                                   uint8_t* mask_out, int32_t* count_out, int32_t* box_out, hipStream_t stream) {
    if (!labels || !mask_out || !count_out || batch <= 0 || batch > 65535 || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 24) || margin < 0)
        return mkd_fail(-1, "region_mask_from_labels: labels [B, H, W] (B <= 65535, H * W <= 2^24), mask and count are required, margin >= 0");
    if (box_classes && !box_out) return mkd_fail(-1, "region_mask_from_labels: box_classes needs box_out [B, 4]");
    hipLaunchKernelGGL(region_init_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, count_out, box_classes ? box_out : nullptr, batch);
    MKD_LAUNCH_CHECK("region_init_kernel");
    if (box_classes) {
        hipLaunchKernelGGL(region_box_kernel, dim3(RM_WGS, batch), dim3(256), 0, stream, labels, H, W, (unsigned long long)box_classes, box_out);
        MKD_LAUNCH_CHECK("region_box_kernel");
    }
    hipLaunchKernelGGL(region_mask_kernel, dim3(RM_WGS, batch), dim3(256), 0, stream, labels, H, W, (unsigned long long)classes,
                       box_classes ? 1 : 0, margin, box_out, mask_out, count_out);
    MKD_LAUNCH_CHECK("region_mask_kernel");
    return 0;
}

size_t hist_match_scratch_bytes(int n) { return n > 0 ? hm_layout(n).total : 0; }

int hist_match_launches(int want_apply, int want_loss) { return 3 + ((want_apply || want_loss) ? 1 : 0) + (want_loss ? 1 : 0); }

int launch_hist_match(const float* dst, const float* ref, const uint8_t* mask_dst, const uint8_t* mask_ref, const int32_t* index, int n, int H,
                      int W, float* matched, uint8_t* tables, float* loss, int32_t* counts, void* scratch, hipStream_t stream) {
    if (!dst || !ref || !mask_dst || !mask_ref || !scratch) return mkd_fail(-1, "hist_match: null pointer");
    if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 24))
        return mkd_fail(-1, "hist_match: 1 <= n <= 65535 terms of [3, H, W] images with H * W <= 2^24");
    if (!matched && !tables && !loss) return mkd_fail(-1, "hist_match: no output requested");
    if (!aligned_to(scratch, 256) || !aligned_to(dst, 4) || !aligned_to(ref, 4)) return mkd_fail(-1, "hist_match: scratch must be 256-byte aligned, images 4-byte aligned");
    const int HW = H * W;
    const HmScratch L = hm_layout(n);
    char* base = (char*)scratch;
    uint32_t* hist = (uint32_t*)(base + L.hist);
    uint8_t* tab_s = (uint8_t*)(base + L.tab);
    int32_t* cnt_s = (int32_t*)(base + L.cnt);
    double* part = (double*)(base + L.part);
    const int vec = (HW % 4 == 0 && aligned_to(dst, 16) && aligned_to(ref, 16) && aligned_to(mask_dst, 4) && aligned_to(mask_ref, 4) &&
                     (!matched || aligned_to(matched, 16))) ? 1 : 0;
    MKD_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n * 2 * 3 * 256 * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(hist_kernel, dim3(HM_WGS, n, 2), dim3(256), 0, stream, dst, ref, mask_dst, mask_ref, index, HW, vec, hist);
    MKD_LAUNCH_CHECK("hist_kernel");
    hipLaunchKernelGGL(table_kernel, dim3(3, n), dim3(256), 0, stream, hist, tab_s, tables, cnt_s, counts);
    MKD_LAUNCH_CHECK("table_kernel");
    if (matched || loss) {
        hipLaunchKernelGGL(apply_kernel, dim3(HM_WGS, n), dim3(256), 0, stream, dst, mask_dst, index, HW, vec, tab_s, cnt_s, matched,
                           loss ? part : nullptr);
        MKD_LAUNCH_CHECK("apply_kernel");
    }
    if (loss) {
        hipLaunchKernelGGL(loss_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, part, n, 3.0 * (double)HW, loss);
        MKD_LAUNCH_CHECK("loss_kernel");
    }
    return 0;
}
