// Counter-based noise on the device (mkd_noise_fill; include/mkd.h holds the definition, tests/noise_ref.py restates it).
//
// Element e of row r of sample b is a pure function of (seed_b, sub_b, stream, r, e): block j = e / 4 is Philox4x32-10 of the counter
// (j, r, stream, sub_b) under the key (seed_b & 0xffffffff, seed_b >> 32), turned into four normals by Box-Muller in DOUBLE and rounded
// to fp32 once.  Nothing is carried from one call to the next and nothing depends on the batch: one launch fills [rows][batch][n].
//
// One thread per block of four elements: the counter is the thread's own index, so there is no shared state, no LDS, no atomics and
// no scratch.  The cost is the double log / sqrt / sincospi (a few million values per call; DESIGN.md section 0 has the numbers).
#include "mkd_common.h"
#include "../../include/mkd.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr int NOISE_NT = 256;

struct Words { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al. 2011; Random123's philox4x32_R with R = 10): ten rounds, the key bumped between them (nine times)
__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Words{{c0, c1, c2, c3}};
}

// u(w) = ((w >> 8) + 0.5) 2^-24: 24 bits and the half, exact in double (not in fp32 above a half), strictly inside (0, 1)
__device__ __forceinline__ double unit_open(uint32_t w) { return ((double)(w >> 8) + 0.5) * 0x1p-24; }

// (rho cospi(2 u_b), rho sinpi(2 u_b)), rho = sqrt(-2 ln u_a): evaluated in double, each rounded to fp32 once
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const double rho = sqrt(-2.0 * log(unit_open(wa)));
    double s, c;
    sincospi(2.0 * unit_open(wb), &s, &c);
    z0 = (float)(rho * c);
    z1 = (float)(rho * s);
}

// grid.x strides over the blocks of four of one (row, sample), grid.y over the rows * batch (row, sample) pairs.
// VEC: out is 16-byte aligned and n % 4 == 0, so every block of four is one aligned 16-byte store; else scalar stores below n.
template <bool VEC>
__global__ void __launch_bounds__(NOISE_NT) noise_fill_kernel(const int64_t* __restrict__ seeds, const int32_t* __restrict__ subs, int batch,
                                                              uint32_t stream_id, uint32_t row0, int64_t pairs, int64_t n, uint32_t nblk,
                                                              int kind, uint32_t* __restrict__ out) {
    for (int64_t rb = blockIdx.y; rb < pairs; rb += gridDim.y) {
        const int b = (int)(rb % batch);
        const uint32_t r = row0 + (uint32_t)(rb / batch);
        const uint64_t seed = (uint64_t)seeds[b];
        const uint32_t sub = subs ? (uint32_t)subs[b] : 0u;
        uint32_t* __restrict__ o = out + rb * n;
        // (64-bit loop index: j + the grid's stride may pass 2^32 where nblk is close to it)
        for (uint64_t j = (uint64_t)blockIdx.x * NOISE_NT + threadIdx.x; j < nblk; j += (uint64_t)gridDim.x * NOISE_NT) {
            Words q = philox4x32_10((uint32_t)j, r, stream_id, sub, (uint32_t)seed, (uint32_t)(seed >> 32));
            if (kind == 0) {
                float z0, z1, z2, z3;
                box_muller(q.w[0], q.w[1], z0, z1);
                box_muller(q.w[2], q.w[3], z2, z3);
                q.w[0] = __float_as_uint(z0);
                q.w[1] = __float_as_uint(z1);
                q.w[2] = __float_as_uint(z2);
                q.w[3] = __float_as_uint(z3);
            }
            const int64_t e = (int64_t)(j * 4);
            if (VEC) {
                *reinterpret_cast<uint4*>(o + e) = make_uint4(q.w[0], q.w[1], q.w[2], q.w[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (e + i < n) o[e + i] = q.w[i];
            }
        }
    }
}

}  // namespace

int mkd_noise_fill(const int64_t* seeds, const int32_t* subs, int batch, uint32_t stream_id, uint32_t row0, int rows, int64_t n_per_sample,
                   int kind, void* out, void* stream) {
    const std::string who = "mkd_noise_fill: ";
    if (!seeds || !out) return mkd_fail(MKD_ERR_ARG, who + "null seeds / out");
    if (batch < 1 || rows < 1 || n_per_sample < 1) return mkd_fail(MKD_ERR_ARG, who + "batch, rows and n_per_sample must be >= 1");
    if (kind != 0 && kind != 1) return mkd_fail(MKD_ERR_ARG, who + "kind must be 0 (normals) or 1 (raw words)");
    const int64_t nblk = n_per_sample / 4 + (n_per_sample % 4 != 0);
    if (nblk > (int64_t)0xffffffffLL) return mkd_fail(MKD_ERR_ARG, who + "ceil(n_per_sample / 4) must fit 32 bits (the block index is one counter word)");
    if ((uint64_t)row0 + (uint64_t)(rows - 1) > 0xffffffffull) return mkd_fail(MKD_ERR_ARG, who + "row0 + rows - 1 must fit 32 bits (the row is one counter word)");
    const int64_t pairs = (int64_t)rows * batch;
    const bool vec = ((uintptr_t)out & 15) == 0 && n_per_sample % 4 == 0;
    int64_t gx = (nblk + NOISE_NT - 1) / NOISE_NT;
    if (gx > 65536) gx = 65536;          // (grid-stride beyond: 2^24 blocks of four per pass)
    const int64_t gy = pairs < 65535 ? pairs : 65535;
    const dim3 grid((unsigned)gx, (unsigned)gy), block(NOISE_NT);
    if (vec)
        hipLaunchKernelGGL(noise_fill_kernel<true>, grid, block, 0, (hipStream_t)stream, seeds, subs, batch, stream_id, row0, pairs, n_per_sample,
                           (uint32_t)nblk, kind, (uint32_t*)out);
    else
        hipLaunchKernelGGL(noise_fill_kernel<false>, grid, block, 0, (hipStream_t)stream, seeds, subs, batch, stream_id, row0, pairs, n_per_sample,
                           (uint32_t)nblk, kind, (uint32_t*)out);
    MKD_LAUNCH_CHECK("noise_fill_kernel");
    return 0;
}
