// Small HBM-bound kernels of the path: DDIM update (+CFG combine), GEGLU, sinusoidal timestep
// embedding, the three tiny-channel 3x3 convs (4->C, 6->16, C->4), weight packing, layout glue.
#include "mkd_common.h"
#include <cstring>

namespace {

// ---- guidance rescale (Lin et al. 2023, section 3.4): the guided eps of element i scaled by its sample's factor ----------------
// The one expression of the engaged path (every step kernel, stand-alone or in the loop): explicit fma, then one multiply, so the
// bits do not depend on what the compiler contracts.  kfac[b] comes from cfg_rescale_factor_kernel.
__device__ __forceinline__ float cfg_rescaled_eps_at(float ec, float eu, float cfg_scale, const float* __restrict__ kfac, int64_t i,
                                                     int n_per_sample) {
    return fmaf(cfg_scale, ec - eu, eu) * kfac[i / n_per_sample];
}
// The guided eps of every solver: model_uncond + s * (model_t - model_uncond), rescaled where the launch has factors (uniform branch)
__device__ __forceinline__ float guided_eps_at(float ec, float eu, float cfg_scale, const float* __restrict__ kfac, int64_t i,
                                               int n_per_sample) {
    return kfac ? cfg_rescaled_eps_at(ec, eu, cfg_scale, kfac, i, n_per_sample) : fmaf(cfg_scale, ec - eu, eu);
}

// One workgroup of 256 threads per sample.  Thread t takes elements t, t + 256, ... of its sample and keeps fp64 sums of e_c, e_c^2,
// g, g^2 (a product of two floats is exact in double); the sums are reduced inside each wave by shuffles (offsets 32 .. 1), then
// thread 0 adds the four waves' values from LDS in wave order: an order fixed by n_per_sample alone, whatever the grid or the loop
// form.  k = phi sqrt(var(e_c) / var(g)) + (1 - phi) in double, rounded once, one store.  var = sum(v^2) - sum(v)^2 / n (the 1 / (n - 1)
// of the unbiased estimate cancels in the ratio); a var(g) that is not above the rounding error of its own sums
// (3 n roundings of 2^-53 at most: 4 n 2^-52 sum(g^2) bounds it) counts as zero: k = 1.  No atomics, no scratch.
__global__ void __launch_bounds__(256) cfg_rescale_factor_kernel(const float* __restrict__ eps_c, const float* __restrict__ eps_u,
                                                                 float cfg_scale, float phi_arg, const StepState* __restrict__ st,
                                                                 int n_per_sample, float* __restrict__ k_out) {
    __shared__ double red[4][4];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* __restrict__ ec = eps_c + (int64_t)b * n_per_sample;
    const float* __restrict__ eu = eps_u + (int64_t)b * n_per_sample;
    double sc = 0.0, scc = 0.0, sg = 0.0, sgg = 0.0;
    for (int i = t; i < n_per_sample; i += 256) {
        const float c = ec[i], u = eu[i];
        const float g = fmaf(cfg_scale, c - u, u);
        sc += (double)c; scc += (double)c * (double)c;
        sg += (double)g; sgg += (double)g * (double)g;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sc += __shfl_down(sc, off, 64); scc += __shfl_down(scc, off, 64);
        sg += __shfl_down(sg, off, 64); sgg += __shfl_down(sgg, off, 64);
    }
    if ((t & 63) == 0) { red[t >> 6][0] = sc; red[t >> 6][1] = scc; red[t >> 6][2] = sg; red[t >> 6][3] = sgg; }
    __syncthreads();
    if (t == 0) {
        double a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
        const double n = (double)n_per_sample;
        const double phi = (double)(st ? st->phi : phi_arg);
        double vc = a[1] - a[0] * a[0] / n, vg = a[3] - a[2] * a[2] / n;
        if (!(vc > 0.0)) vc = 0.0;
        double k = 1.0;
        if (vg > 4.0 * n * 2.220446049250313e-16 * a[3]) k = phi * sqrt(vc / vg) + (1.0 - phi);
        k_out[b] = (float)k;
    }
}

// ---- DDIM x0 / x_{t-1} update, reference diffmk/cddim.py:39-40 (CFG) and :63,74-78 ----------------
// One element, the ONE expression of every form of the DDIM step kernel: (after the guided eps, guided_eps_at above) x0 and
// x_{t-1}, then the eta term.  The library is built with -ffp-contract=fast, and what the compiler fuses depends on the code around
// an expression (a 16-byte loop body fused sqrt(a_prev) x0 + dir e into an fma for two of its four elements, a scalar one for none),
// so every rounding is spelled out: explicit fmas, and the two products of the sum pass through an empty asm statement (no
// instruction; the value is opaque and cannot be folded into an fma).  These are the operations the scalar uniform kernels compiled to
// before they were spelled out.
__device__ __forceinline__ float ddim_keep_product(float p) { asm("" : "+v"(p)); return p; }
__device__ __forceinline__ float ddim_update_at(float xv, float e, const DdimCoef& k, float& p0) {
    p0 = fmaf(-k.s1m, e, xv) * k.sqrt_at_inv;          // (x - sqrt(1-a_t) e) / sqrt(a_t)
    return ddim_keep_product(k.sqrt_aprev * p0) + ddim_keep_product(k.dir_coef * e);      // sqrt(a_prev) x0 + sqrt(1-a_prev-sigma^2) e
}
__device__ __forceinline__ float ddim_noise_at(float xp, float sigma, float nz, float temperature) { return fmaf(sigma * nz, temperature, xp); }

// ---- device-resident step state for hipGraph replay of the DDIM loop -------------------------------------
// One graph = one reverse step; what changes between steps (timestep, schedule coefficients) is read from
// device tables through a counter that the first kernel of the graph advances, so the SAME graph replays.
__device__ __forceinline__ void temb_copy_rows(const TembSel& ts, int step, int gtid, int gthreads) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int nv = ts.n[k] >> 2;
        if (!nv) continue;
        const f32x4* src = (const f32x4*)(ts.tab[k] + (size_t)step * ts.n[k]);
        f32x4* dst = (f32x4*)ts.proj[k];
        for (int i = gtid; i < nv * ts.batch; i += gthreads) dst[i] = src[i % nv];
    }
}

// ---- masked sampling (UPSTREAM DDIMSampler.ddim_sampling: img = q_sample(x0, ts) * mask + (1 - mask) * img) ------------------
// Element i of a [B, C, hw] latent; the mask is read at b * mbs + c * mcs + p (stride 0 broadcasts).  mask null: the q_sample alone.
// Explicit fmas: the loop kernel and the stand-alone kernel give the same bits whatever the compiler contracts.
__device__ __forceinline__ float q_sample_blend_at(const float* __restrict__ x0, const float* __restrict__ nz, const float* __restrict__ mask,
                                                   const float* img, float sa, float s1m, int64_t i, int hw, int chw, int mbs, int mcs) {
    const float q = fmaf(sa, x0[i], s1m * nz[i]);
    if (!mask) return q;
    const int64_t b = i / chw;
    const int r = (int)(i - b * chw);
    const int c = r / hw;
    const float m = mask[b * mbs + (int64_t)c * mcs + (r - c * hw)];
    return fmaf(m, q, (1.0f - m) * img[i]);
}

__global__ void q_sample_blend_kernel(const float* __restrict__ x0, const float* __restrict__ nz, float sa, float s1m,
                                      const float* __restrict__ mask, const float* x, float* out, int64_t n, int hw, int chw, int mbs, int mcs) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = q_sample_blend_at(x0, nz, mask, x, sa, s1m, i, hw, chw, mbs, mcs);
}

// ---- uint8 label map -> latent mask: fraction of each f x f block whose label is in the class set (area average) ----------------
__global__ void latent_mask_from_labels_kernel(const uint8_t* __restrict__ labels, int batch, int H, int W, unsigned long long classes,
                                               int f, float threshold, float* __restrict__ out) {
    const int h = H / f, w = W / f;
    const int64_t total = (int64_t)batch * h * w;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(o % w), y = (int)((o / w) % h);
        const int64_t b = o / ((int64_t)h * w);
        const uint8_t* src = labels + (b * H + (int64_t)y * f) * W + (int64_t)x * f;
        int cnt = 0;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) {
                const unsigned l = src[(int64_t)dy * W + dx];
                cnt += (l < 64u) ? (int)((classes >> l) & 1ull) : 0;
            }
        const float frac = (float)cnt / (float)(f * f);
        out[o] = threshold > 0.f ? (frac >= threshold ? 1.0f : 0.0f) : frac;
    }
}

__global__ void step_setup_kernel(StepState* st, int64_t* t_out, int batch, const TembSel ts, float* x, int64_t n) {
    const int i = st->counter;          // read-only in this kernel: the solver's step kernel, the step's last, advances it
    if (blockIdx.x == 0) {
        for (int b = threadIdx.x; b < batch; b += blockDim.x) t_out[b] = st->timesteps[i];
        if (threadIdx.x == 0) st->cur_row = st->n_steps - 1 - i;          // the executed step: all the step's last kernel is told
    }
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gthreads = gridDim.x * blockDim.x;
    temb_copy_rows(ts, i, gtid, gthreads);
    const float* x0 = st->x0;
    if (x0) {           // masked: this step's blend.  Coefficients and noise row from the tables through the counter, never from
                        // cur_row, which block 0 of this same kernel writes while the other blocks run
        const float sa = st->q[2 * i], s1m = st->q[2 * i + 1];
        const float* nz = st->q_noise + (int64_t)(st->n_steps - 1 - i) * n;
        const float* mask = st->mask;
        const int hw = st->q_hw, chw = st->q_chw, mbs = st->mask_bstride, mcs = st->mask_cstride;
        for (int64_t k = gtid; k < n; k += gthreads) x[k] = q_sample_blend_at(x0, nz, mask, x, sa, s1m, k, hw, chw, mbs, mcs);
    }
}

__global__ void temb_select_kernel(const TembSel ts, int step) {
    temb_copy_rows(ts, step, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// ---- DPM-Solver++ multistep update (Lu et al. 2022, Algorithm 2; data prediction, eps parameterisation) -----------------------
// One element: m0 = (x - sigma_t e) / alpha_t, x' = c_x x + c_0 m0 + c_1 m1 + c_2 m2.  Explicit fmas (at most eight roundings with the
// guidance combine): every form of the step kernel gives the same bits whatever the compiler contracts.
__device__ __forceinline__ float dpmpp_update_at(float x, float e, const DpmCoef& k, float m1, float m2, float& m0) {
    m0 = fmaf(-k.sigma, e, x) * k.inv_alpha;
    float r = fmaf(k.c0, m0, k.cx * x);
    if (k.c1 != 0.f) r = fmaf(k.c1, m1, r);
    if (k.c2 != 0.f) r = fmaf(k.c2, m2, r);
    return r;
}
// ---- UniPC predictor-corrector update (Zhao et al. 2023; data prediction, the linear forms of include/mkd.h mkd_unipc_table) ----
// One element, with x = x~_k the predicted latent the model was evaluated at and xcp = x^c_{k-1} the previous corrected one:
//   m0 = (x - sigma_t e) / alpha_t
//   xc = a_c xcp + q_0 m0 + q_1 m1 + q_2 m2 + q_3 m3      (a_c == 0: no corrector in this step, xc = x)
//   x' = a_p xc + p_0 m0 + p_1 m1 + p_2 m2
// Explicit fmas (two roundings of the guidance combine, two of m0, at most five of xc, four of x'): every form of the step kernel
// gives the same bits whatever the compiler contracts.  A history term is added only where its coefficient is non-zero.
__device__ __forceinline__ float unipc_update_at(float x, float xcp, float e, const UniCoef& k, float m1, float m2, float m3, float& m0,
                                                 float& xc) {
    m0 = fmaf(-k.sigma, e, x) * k.inv_alpha;
    float c = x;
    if (k.ac != 0.f) {
        c = fmaf(k.q0, m0, k.ac * xcp);
        if (k.q1 != 0.f) c = fmaf(k.q1, m1, c);
        if (k.q2 != 0.f) c = fmaf(k.q2, m2, c);
        if (k.q3 != 0.f) c = fmaf(k.q3, m3, c);
    }
    xc = c;
    float r = fmaf(k.p0, m0, k.ap * c);
    if (k.p1 != 0.f) r = fmaf(k.p1, m1, r);
    if (k.p2 != 0.f) r = fmaf(k.p2, m2, r);
    return r;
}
// ---- per-sample loop (mkd_sample_rows): every sample of the batch has its own schedule, guidance scale and sigmas -------------------
// Grid (x, sample): what a workgroup needs of its sample (one StepRow) has a workgroup-uniform address, so it is read once into
// scalars, and no element is divided by the sample size.  The updates are the per-sample forms of the step kernels below: row b has the bits of
// the uniform forms run with sample b's numbers.
//
// First kernel of a per-sample step.  Block (0, b) writes t_out[b]; every block copies its share of row b's time-embedding rows (row
// temb_row of sample b % samples: with guidance both halves of the doubled batch take their sample's row).  The executed step k goes
// to st->cur_row for the step's last kernel, which moves the counter (read-only here, as in step_setup_kernel).
__global__ void step_setup_rows_kernel(StepState* st, int64_t* t_out, int samples, const TembSel ts) {
    const int k = st->n_steps - 1 - st->counter;
    const int b = blockIdx.y;
    const StepRow* __restrict__ r = st->rows + (int64_t)k * samples + (b % samples);
    const int64_t t = r->t;
    const int row = r->temb_row;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t_out[b] = t;
        if (b == 0) st->cur_row = k;
    }
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gthreads = gridDim.x * blockDim.x;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int nv = ts.n[j] >> 2;
        if (!nv) continue;
        const f32x4* __restrict__ src = (const f32x4*)(ts.tab[j] + (size_t)row * ts.n[j]);
        f32x4* __restrict__ dst = (f32x4*)(ts.proj[j] + (size_t)b * ts.n[j]);
        for (int i = gtid; i < nv; i += gthreads) dst[i] = src[i];
    }
}

// ---- the step kernels: one walker, one kernel per solver, every form of StepOps (mkd_common.h) ------------------------------------
// What a block walks over once its launch's record is resolved: the common operands at this block's elements (the whole latent, or
// one sample's slice), and where the launch stands: executed step k / table entry e of the st forms, the sample's row and offset
// of the per-sample forms (row null, off 0 otherwise)
struct StepRange {
    const float* x; const float* eps_c; const float* eps_u; float scale; const float* kfac; int per; int64_t n;
    float* x_out; float* p_out; float* x_copy; float* p_copy;
    int k, e; const StepRow* row; int64_t off;
};
// A solver is an element functor F: its numbers k, up to four extra input planes `in` (null: not read), with F::XC an extra output
// plane xc_out, and
//   float at(x, e, h, p0, xc)      the new latent of one element from x, the guided eps e and the planes' values h[] (0 where not
//                                  read); p0 = its x0-prediction, xc = the corrected latent (F::XC only)
// The walker owns everything else: the grid stride over r.n elements, the guided eps, the loads of the planes that are read and the
// stores of x_out / p_out (/ xc_out), the first two once more where a copy is asked for.  W = 4: 16-byte accesses, W = 1: scalar, the
// same arithmetic per element.  Every load of element i comes before its stores, so x_out may be x and xc_out may be in[0]: no
// __restrict__ on those.  A plane is read only where its pointer is non-null: the branch is uniform, so a first step or a lower order
// issues no loads for history it does not use.
template <int W, class F>
__device__ __forceinline__ void step_walk_as(const StepRange& r, const F& f) {
    typedef float vec __attribute__((ext_vector_type(W)));
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < r.n / W; i += nth) {
        const vec xv = ((const vec*)r.x)[i];
        vec ev = ((const vec*)r.eps_c)[i], hv[F::PLANES], rv, pv, cv;
        if (r.eps_u) {
            const vec uv = ((const vec*)r.eps_u)[i];
#pragma unroll
            for (int j = 0; j < W; ++j) ev[j] = guided_eps_at(ev[j], uv[j], r.scale, r.kfac, W * i + j, r.per);
        }
#pragma unroll
        for (int p = 0; p < F::PLANES; ++p) hv[p] = f.in[p] ? ((const vec*)f.in[p])[i] : (vec)0.f;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            float h[F::PLANES], p0, xc = 0.f;
#pragma unroll
            for (int p = 0; p < F::PLANES; ++p) h[p] = hv[p][j];
            rv[j] = f.at(xv[j], ev[j], h, p0, xc);
            pv[j] = p0; cv[j] = xc;
        }
        if (r.p_out) ((vec*)r.p_out)[i] = pv;
        if constexpr (F::XC) ((vec*)f.xc_out)[i] = cv;
        ((vec*)r.x_out)[i] = rv;
        if (r.p_copy) ((vec*)r.p_copy)[i] = pv;
        if (r.x_copy) ((vec*)r.x_copy)[i] = rv;
    }
}
// 16-byte form when n is a multiple of 4 and every pointer that is used is 16-byte aligned (null ones count as aligned), else scalar
template <class F>
__device__ __forceinline__ void step_walk(const StepRange& r, const F& f) {
    uintptr_t al = (uintptr_t)r.x | (uintptr_t)r.eps_c | (uintptr_t)r.eps_u | (uintptr_t)r.x_out | (uintptr_t)r.p_out | (uintptr_t)r.x_copy |
                   (uintptr_t)r.p_copy;
#pragma unroll
    for (int p = 0; p < F::PLANES; ++p) al |= (uintptr_t)f.in[p];
    if constexpr (F::XC) al |= (uintptr_t)f.xc_out;
    if (!(r.n & 3) && !(al & 15)) step_walk_as<4>(r, f);
    else step_walk_as<1>(r, f);
}

// What all solvers resolve alike.  st forms: the executed step, the trace rows (uniform launches) and the counter, which this last
// kernel of the step moves and nothing in it reads.  Per-sample forms: this block's StepRow and its sample's slice of the operands.
// false: a finished sample, whose blocks return before any access to its rows.
__device__ __forceinline__ bool step_resolve(const StepOps& o, StepRange& r) {
    StepState* const st = o.st;
    const int k = st ? st->cur_row : 0, e = st ? st->n_steps - 1 - k : 0;
    const bool traced = st && !o.samples && st->trace_row[e] >= 0;
    const int64_t trace_at = traced ? st->trace_row[e] * o.n : 0;
    if (st && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) st->counter = st->counter - 1;
    const StepRow* const row = o.samples ? (st ? st->rows + (int64_t)k * o.samples : o.rows) + blockIdx.y : nullptr;
    if (row && !row->active) return false;
    const int64_t off = row ? (int64_t)blockIdx.y * o.per : 0;
    r.x = o.x + off; r.eps_c = o.eps_c + off; r.eps_u = o.eps_u ? o.eps_u + off : nullptr;
    r.scale = row ? row->scale : o.scale; r.kfac = o.kfac; r.per = o.per; r.n = row ? o.per : o.n;
    r.x_out = o.x_out + off; r.p_out = o.p_out ? o.p_out + off : nullptr;
    r.x_copy = st ? (traced && st->trace_x ? st->trace_x + trace_at : nullptr) : o.x_copy;
    r.p_copy = st ? (traced && st->trace_x0 ? st->trace_x0 + trace_at : nullptr) : o.p_copy;
    r.k = k; r.e = e; r.row = row; r.off = off;
    return true;
}

// DDIM.  Plane 0: the noise draw of the eta term.  The st forms take the executed step's row of st->noise; a table entry or a sample's
// row with sigma == 0 reads none
struct DdimStep {
    static constexpr int PLANES = 1; static constexpr bool XC = false;
    DdimCoef k; float sigma, temperature; const float* in[PLANES];
    __device__ __forceinline__ float at(float x, float e, const float* h, float& p0, float&) const {
        const float xp = ddim_update_at(x, e, k, p0);
        return in[0] ? ddim_noise_at(xp, sigma, h[0], temperature) : xp;
    }
};
__global__ void ddim_step_kernel(const StepOps o) {
    StepRange r;
    if (!step_resolve(o, r)) return;
    const StepState* const st = o.st;
    DdimStep f;
    f.k = r.row ? DdimCoef::from(r.row->coef) : st ? DdimCoef::from(st->coef + 4 * r.e) : DdimCoef::from(o.coef);
    f.sigma = r.row ? r.row->sigma : st ? st->sigma[r.e] : o.sigma;
    f.temperature = st ? st->temperature : o.temperature;
    const float* const nz = st ? (st->noise ? st->noise + r.k * o.n : nullptr) : o.noise;
    f.in[0] = (nz && !((r.row || st) && f.sigma == 0.f)) ? nz + r.off : nullptr;
    step_walk(r, f);
}

// DPM-Solver++.  Planes m_{k-1}, m_{k-2}; the st forms keep them and m_k = p_out in the three-plane ring
struct DpmStep {
    static constexpr int PLANES = 2; static constexpr bool XC = false;
    DpmCoef k; const float* in[PLANES];
    __device__ __forceinline__ float at(float x, float e, const float* h, float& p0, float&) const { return dpmpp_update_at(x, e, k, h[0], h[1], p0); }
};
__global__ void dpmpp_step_kernel(const StepOps o) {
    StepRange r;
    if (!step_resolve(o, r)) return;
    const StepState* const st = o.st;
    DpmStep f;
    f.k = r.row ? DpmCoef::from(r.row->dpm) : st ? DpmCoef::from(st->dpm + 6 * r.e) : DpmCoef::from(o.coef);
    if (st) r.p_out = st->ring + ring_slot(r.k, 0, 3) * o.n + r.off;
    f.in[0] = f.k.c1 != 0.f ? (st ? st->ring + ring_slot(r.k, 1, 3) * o.n : o.hist[0]) + r.off : nullptr;
    f.in[1] = f.k.c2 != 0.f ? (st ? st->ring + ring_slot(r.k, 2, 3) * o.n : o.hist[1]) + r.off : nullptr;
    step_walk(r, f);
}

// UniPC.  Planes x^c_{k-1}, m_{k-1}, m_{k-2}, m_{k-3}, each read only where a coefficient of its own is non-zero; the st form keeps the
// m's in the four-plane ring and x^c in place in st->xc.  No per-sample form
struct UniStep {
    static constexpr int PLANES = 4; static constexpr bool XC = true;
    UniCoef k; const float* in[PLANES]; float* xc_out;
    __device__ __forceinline__ float at(float x, float e, const float* h, float& p0, float& xc) const {
        return unipc_update_at(x, h[0], e, k, h[1], h[2], h[3], p0, xc);
    }
};
__global__ void unipc_step_kernel(const StepOps o) {
    StepRange r;
    if (!step_resolve(o, r)) return;
    const StepState* const st = o.st;
    UniStep f;
    f.k = st ? UniCoef::from(st->uni + 12 * r.e) : UniCoef::from(o.coef);
    if (st) r.p_out = st->ring + ring_slot(r.k, 0, 4) * o.n;
    f.xc_out = st ? st->xc : o.xc_out;
    const bool cor = f.k.ac != 0.f;
    f.in[0] = cor ? (st ? st->xc : o.xc_prev) : nullptr;
    f.in[1] = ((cor && f.k.q1 != 0.f) || f.k.p1 != 0.f) ? (st ? st->ring + ring_slot(r.k, 1, 4) * o.n : o.hist[0]) : nullptr;
    f.in[2] = ((cor && f.k.q2 != 0.f) || f.k.p2 != 0.f) ? (st ? st->ring + ring_slot(r.k, 2, 4) * o.n : o.hist[1]) : nullptr;
    f.in[3] = (cor && f.k.q3 != 0.f) ? (st ? st->ring + ring_slot(r.k, 3, 4) * o.n : o.hist[2]) : nullptr;
    step_walk(r, f);
}

// ---- GEGLU: y = a * gelu_erf(gate) ----------------------------------------------------------------
__global__ void geglu_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int rows, int inner) {
    const int vper = inner >> 3;
    const int64_t total = (int64_t)rows * vper;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx / vper);
        const int c = (int)(idx - (int64_t)r * vper) << 3;
        const U16x8 a = *(const U16x8*)(x + (size_t)r * 2 * inner + c);
        const U16x8 gt = *(const U16x8*)(x + (size_t)r * 2 * inner + inner + c);
        U16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = f32_to_bf16(bf16_to_f32(a.v[j]) * gelu_erf_f(bf16_to_f32(gt.v[j])));
        *(U16x8*)(y + (size_t)r * inner + c) = o;
    }
}

// ---- sinusoidal timestep embedding: out[b] = [cos(t f_k), sin(t f_k)], f_k = exp(-ln(1e4) k / half) --
__global__ void timestep_embedding_kernel(const int64_t* __restrict__ t, bf16_t* __restrict__ out, int batch, int dim) {
    const int half = dim >> 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * half) return;
    const int b = idx / half, k = idx - b * half;
    const float freq = expf(-9.210340371976184f * (float)k / (float)half);
    const float a = (float)t[b] * freq;
    out[(size_t)b * dim + k] = f32_to_bf16(cosf(a));
    out[(size_t)b * dim + half + k] = f32_to_bf16(sinf(a));
}

// ---- direct 3x3 conv (pad 1), one thread per output element, fp32 accumulate ----------------------
// Only used where the channel count is too small for the MFMA path (Cin 4/6, or Cout 4).
__global__ void conv3x3_direct_kernel(const void* __restrict__ xin, int in_nchw_f32, const bf16_t* __restrict__ w,
                                      const float* __restrict__ bias, void* __restrict__ yout, int out_nchw_f32,
                                      int act, const bf16_t* __restrict__ add, int batch, int Hin, int Win,
                                      int Cin, int Cout, int Hout, int Wout, int stride) {
    const int64_t total = (int64_t)batch * Hout * Wout * Cout;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(idx % Cout);
        int64_t pix = idx / Cout;
        const int ox = (int)(pix % Wout); pix /= Wout;
        const int oy = (int)(pix % Hout);
        const int b = (int)(pix / Hout);
        float acc = bias ? bias[co] : 0.f;
        const bf16_t* wr = w + (size_t)co * 9 * Cin;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * stride + ky - 1;
            if ((unsigned)iy >= (unsigned)Hin) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * stride + kx - 1;
                if ((unsigned)ix >= (unsigned)Win) continue;
                const bf16_t* wt = wr + (ky * 3 + kx) * Cin;
                if (in_nchw_f32) {
                    const float* xp = (const float*)xin + ((size_t)b * Cin * Hin + iy) * Win + ix;
                    for (int ci = 0; ci < Cin; ++ci)
                        acc += xp[(size_t)ci * Hin * Win] * bf16_to_f32(wt[ci]);
                } else {
                    const bf16_t* xp = (const bf16_t*)xin + ((size_t)(b * Hin + iy) * Win + ix) * Cin;
                    for (int ci = 0; ci < Cin; ++ci) acc += bf16_to_f32(xp[ci]) * bf16_to_f32(wt[ci]);
                }
            }
        }
        if (act == 1) acc = silu_f(acc);
        const size_t opix = ((size_t)b * Hout + oy) * Wout + ox;
        if (add) acc += bf16_to_f32(add[opix * Cout + co]);
        if (out_nchw_f32) ((float*)yout)[(((size_t)b * Cout + co) * Hout + oy) * Wout + ox] = acc;
        else ((bf16_t*)yout)[opix * Cout + co] = f32_to_bf16(acc);
    }
}

// ---- 3x3 conv with a tiny Cin read from fp32 NCHW (the 4 -> 320 input conv): thread = output channel, the
// thread's 9*CIN weights live in registers, a block walks pixels with the 9*CIN input patch shared through LDS.
template <int CIN>
__global__ __launch_bounds__(512) void conv3x3_fewin_kernel(const float* __restrict__ x, const Pair<ConvInIo> io, int act, int batch, int H, int W,
                                                            int Cout, int pix_per_block) {
    // grouped launch: grid y selects the problem (both nets convolve the SAME x with their own weights)
    const bf16_t* __restrict__ const w = io.g[blockIdx.y].w; const float* __restrict__ const bias = io.g[blockIdx.y].bias;
    bf16_t* __restrict__ const y = io.g[blockIdx.y].y; const bf16_t* __restrict__ const add = io.g[blockIdx.y].add;
    constexpr int KK = 9 * CIN;
    constexpr int PPB_MAX = 16;
    __shared__ float patch[PPB_MAX][KK];
    const int co = threadIdx.x;
    const bool live = co < Cout;
    float wr[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) wr[k] = live ? bf16_to_f32(w[(size_t)co * KK + k]) : 0.f;
    const float bz = (live && bias) ? bias[co] : 0.f;
    const int npix = batch * H * W;
    const int p0 = blockIdx.x * pix_per_block;
    const int p1 = min(npix, p0 + pix_per_block);
    // every input patch of the block's pixels in ONE round of loads (a per-pixel prefetch only covers one iteration, ~0.1 us,
    // of a ~1 us load latency: the old loop paid that latency per pixel)
    for (int idx = threadIdx.x; idx < (p1 - p0) * KK; idx += blockDim.x) {
        const int pp = idx / KK, k = idx - pp * KK;
        const int tap = k / CIN, ci = k - tap * CIN;
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int pix = p0 + pp;
        const int b = pix / (H * W);
        const int rem = pix - b * H * W;
        const int oy = rem / W, ox = rem - oy * W;
        const int iy = oy + ky - 1, ix = ox + kx - 1;
        float v = 0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = x[(((size_t)b * CIN + ci) * H + iy) * W + ix];
        patch[pp][k] = v;
    }
    __syncthreads();
    if (!live) return;
    for (int pix = p0; pix < p1; ++pix) {
        float acc = bz;
#pragma unroll
        for (int k = 0; k < KK; ++k) acc += patch[pix - p0][k] * wr[k];
        if (act == 1) acc = silu_f(acc);
        if (add) acc += bf16_to_f32(add[(size_t)pix * Cout + co]);
        y[(size_t)pix * Cout + co] = f32_to_bf16(acc);
    }
}

// ---- 3x3 conv with a tiny Cout (the UNet's final C -> 4): one wavefront per output pixel ---------------
// lanes split the (tap, ci) reduction in 16-B vectors, COUT accumulators per lane, wave-shuffle tree at the end.
template <int COUT>
__global__ __launch_bounds__(256) void conv3x3_fewout_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y_nchw,
                                                             int batch, int H, int W, int Cin) {
    const int lane = threadIdx.x & 63;
    const int pix = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int npix = batch * H * W;
    if (pix >= npix) return;
    const int b = pix / (H * W);
    const int rem = pix - b * H * W;
    const int oy = rem / W, ox = rem - oy * W;
    const int V = Cin >> 3;
    float acc[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) acc[c] = 0.f;
    for (int idx = lane; idx < 9 * V; idx += 64) {
        const int tap = idx / V, v = idx - tap * V;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;
        const int iy = oy + ky - 1, ix = ox + kx - 1;
        if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
        const U16x8 xv = *(const U16x8*)(x + ((size_t)(b * H + iy) * W + ix) * Cin + v * 8);
        float xf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[j] = bf16_to_f32(xv.v[j]);
#pragma unroll
        for (int c = 0; c < COUT; ++c) {
            const U16x8 wv = *(const U16x8*)(w + ((size_t)c * 9 + tap) * Cin + v * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[c] += xf[j] * bf16_to_f32(wv.v[j]);
        }
    }
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
        float a = acc[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) y_nchw[(((size_t)b * COUT + c) * H + oy) * W + ox] = a + (bias ? bias[c] : 0.f);
    }
}

// ---- fused tail of the VAE encoder (UPSTREAM Encoder.conv_out -> AutoencoderKL.quant_conv -> DiagonalGaussianDistribution ->
// sample() / mode() -> get_first_stage_encoding's x scale_factor): one wavefront per latent pixel.  conv_out (3x3 pad 1, Cin -> 2Z,
// bf16 NHWC in) is reduced as in conv3x3_fewout_kernel; then lane 0 holds the 2Z conv outputs and applies quant_conv (a 2Z x 2Z
// matrix-vector product in registers): moments = (mean | logvar), std = exp(0.5 clamp(logvar, -30, 20)),
// z = (mean + std * noise) * scale (noise == null: mode() = mean).  z [B,Z,h,w] and moments [B,2Z,h,w] fp32 NCHW, either may be null.
template <int Z>
__global__ __launch_bounds__(256) void vae_enc_tail_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                           const float* __restrict__ bias, const bf16_t* __restrict__ wq,
                                                           const float* __restrict__ bq, const float* __restrict__ noise, float scale,
                                                           float* __restrict__ z_out, float* __restrict__ mom_out,
                                                           int batch, int H, int W, int Cin) {
    constexpr int C2 = 2 * Z;
    const int lane = threadIdx.x & 63;
    const int pix = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int npix = batch * H * W;
    if (pix >= npix) return;
    const int b = pix / (H * W);
    const int rem = pix - b * H * W;
    const int oy = rem / W, ox = rem - oy * W;
    const int V = Cin >> 3;
    float acc[C2];
#pragma unroll
    for (int c = 0; c < C2; ++c) acc[c] = 0.f;
    for (int idx = lane; idx < 9 * V; idx += 64) {
        const int tap = idx / V, v = idx - tap * V;
        const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;
        const int iy = oy + ky - 1, ix = ox + kx - 1;
        if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
        const U16x8 xv = *(const U16x8*)(x + ((size_t)(b * H + iy) * W + ix) * Cin + v * 8);
        float xf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[j] = bf16_to_f32(xv.v[j]);
#pragma unroll
        for (int c = 0; c < C2; ++c) {
            const U16x8 wv = *(const U16x8*)(w + ((size_t)c * 9 + tap) * Cin + v * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[c] += xf[j] * bf16_to_f32(wv.v[j]);
        }
    }
#pragma unroll
    for (int c = 0; c < C2; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
        acc[c] += bias[c];
    }
    if (lane != 0) return;
    float m[C2];
#pragma unroll
    for (int o = 0; o < C2; ++o) {
        float s = bq[o];
#pragma unroll
        for (int i = 0; i < C2; ++i) s += bf16_to_f32(wq[o * C2 + i]) * acc[i];
        m[o] = s;
    }
    const size_t hw = (size_t)H * W, p = (size_t)oy * W + ox;
    if (mom_out) {
#pragma unroll
        for (int o = 0; o < C2; ++o) mom_out[((size_t)b * C2 + o) * hw + p] = m[o];
    }
    if (z_out) {
#pragma unroll
        for (int c = 0; c < Z; ++c) {
            float v = m[c];
            if (noise) {
                const float lv = fminf(fmaxf(m[Z + c], -30.0f), 20.0f);
                v += expf(0.5f * lv) * noise[((size_t)b * Z + c) * hw + p];
            }
            z_out[((size_t)b * Z + c) * hw + p] = v * scale;
        }
    }
}

// ---- row softmax, fp32 [rows, cols] in -> bf16 probabilities out (VAE mid-block attention scores), one 256-thread block per row.
// The scores stay fp32 from the Q.K^T accumulator to here: a bf16 logit of magnitude 16..32 is off by up to 2^-4, i.e. several percent
// in every probability of its row (tests/vae_attn_ref.py measures both orders of rounding).
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, int cols) {
    __shared__ float red[4];
    const float* xr = x + (size_t)blockIdx.x * cols;
    bf16_t* yr = y + (size_t)blockIdx.x * cols;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float mx = -INFINITY;
    for (int c = threadIdx.x; c < cols; c += 256) mx = fmaxf(mx, xr[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int c = threadIdx.x; c < cols; c += 256) sum += __expf(xr[c] - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) red[wv] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    for (int c = threadIdx.x; c < cols; c += 256) yr[c] = f32_to_bf16(__expf(xr[c] - mx) * inv);
}

// ---- post_quant_conv: 1x1 conv over fp32 NCHW latents with the 1/scale_factor of decode_first_stage folded in -------
__global__ void post_quant_kernel(const float* __restrict__ z, const bf16_t* __restrict__ w, const float* __restrict__ bias,
                                  float inv_scale, float* __restrict__ out, int batch, int C, int hw) {
    const int64_t total = (int64_t)batch * C * hw;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(idx % hw);
        const int co = (int)((idx / hw) % C);
        const int b = (int)(idx / ((int64_t)hw * C));
        float acc = bias ? bias[co] : 0.f;
        for (int ci = 0; ci < C; ++ci) acc += bf16_to_f32(w[co * C + ci]) * (z[((size_t)b * C + ci) * hw + p] * inv_scale);
        out[idx] = acc;
    }
}

// ---- per-sample blend of two bf16 tensors: y = (1 - alpha[b]) * a + alpha[b] * b (makeup interpolation) ---------------
__global__ void blend_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, const float* __restrict__ alpha,
                             bf16_t* __restrict__ y, int64_t per_sample, int batch) {
    const int64_t total = per_sample * batch / 8;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const float al = alpha[(idx * 8) / per_sample];
        const U16x8 va = *(const U16x8*)(a + idx * 8);
        const U16x8 vb = *(const U16x8*)(b + idx * 8);
        U16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = f32_to_bf16((1.0f - al) * bf16_to_f32(va.v[j]) + al * bf16_to_f32(vb.v[j]));
        *(U16x8*)(y + idx * 8) = o;
    }
}

// ---- fp32 [Cout,Cin,kh,kw] -> bf16 [Cout][kh][kw][Cin] ----------------------------------------------
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int Cout, int Cin, int kh, int kw) {
    const int64_t total = (int64_t)Cout * Cin * kh * kw;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(idx % Cin);
        int64_t r = idx / Cin;
        const int x = (int)(r % kw); r /= kw;
        const int y = (int)(r % kh);
        const int co = (int)(r / kh);
        out[idx] = f32_to_bf16(w[(((size_t)co * Cin + ci) * kh + y) * kw + x]);
    }
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = f32_to_bf16(x[i]);
}

__global__ void bf16_to_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = bf16_to_f32(x[i]);
}

// CLIP text embeddings: out[b, t, :] = token_embedding[tokens[b, t]] + position_embedding[t]   (8 channels per thread)
__global__ void clip_embed_kernel(const int32_t* __restrict__ tokens, const bf16_t* __restrict__ tok_emb,
                                  const bf16_t* __restrict__ pos_emb, bf16_t* __restrict__ out, int rows, int T, int width, int vocab) {
    const int vper = width >> 3;
    const int64_t total = (int64_t)rows * vper;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx / vper);
        const int c = (int)(idx - (int64_t)r * vper) << 3;
        int id = tokens[r];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);        // the host wrapper rejects out-of-range ids; never read OOB
        const U16x8 a = *(const U16x8*)(tok_emb + (size_t)id * width + c);
        const U16x8 b = *(const U16x8*)(pos_emb + (size_t)(r % T) * width + c);
        U16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = f32_to_bf16(bf16_to_f32(a.v[j]) + bf16_to_f32(b.v[j]));
        *(U16x8*)(out + (size_t)r * width + c) = o;
    }
}

// Load-time fold of the transformer's last two linear maps: out = proj_out(h2 + FF2(gg)) + x_in
//   = [gg | h2] . [P.W2 | P]^T + (P.b2 + bp) + x_in      (P = proj_out [d,d], W2 = ff.net.2 [d,4d]; fp32 product, bf16 result)
__global__ void merge_ff_out_kernel(const float* __restrict__ P, const float* __restrict__ W2, const float* __restrict__ b2,
                                    const float* __restrict__ bp, bf16_t* __restrict__ Wm, float* __restrict__ bias_m, int d) {
    const int n = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int K4 = 4 * d;
    if (k < K4) {
        float a = 0.f;
        for (int j = 0; j < d; ++j) a += P[(size_t)n * d + j] * W2[(size_t)j * K4 + k];
        Wm[(size_t)n * 5 * d + k] = f32_to_bf16(a);
    } else if (k < 5 * d) {
        Wm[(size_t)n * 5 * d + k] = f32_to_bf16(P[(size_t)n * d + (k - K4)]);
    }
    if (k == 0) {
        float a = bp[n];
        for (int j = 0; j < d; ++j) a += P[(size_t)n * d + j] * b2[j];
        bias_m[n] = a;
    }
}

__global__ void copy_strided_kernel(const bf16_t* __restrict__ src, int ld_src, bf16_t* __restrict__ dst, int ld_dst,
                                    int rows, int cols) {
    const int vper = cols >> 3;
    const int64_t total = (int64_t)rows * vper;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx / vper);
        const int c = (int)(idx - (int64_t)r * vper) << 3;
        *(U16x8*)(dst + (size_t)r * ld_dst + c) = *(const U16x8*)(src + (size_t)r * ld_src + c);
    }
}

__global__ void repeat_batch_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n_per, int reps) {
    const int64_t total = n_per * reps;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = x[i % n_per];
}

__global__ void fill_i64_kernel(int64_t* p, int64_t v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

inline int grid_for(int64_t total, int block = 256, int cap = 2048) {
    int64_t g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

int launch_geglu(const bf16_t* x, bf16_t* y, int rows, int inner, hipStream_t stream) {
    if (inner % 8) return mkd_fail(-1, "geglu: inner must be a multiple of 8");
    hipLaunchKernelGGL(geglu_kernel, dim3(grid_for((int64_t)rows * (inner / 8), 256, 4096)), dim3(256), 0, stream, x, y, rows, inner);
    MKD_LAUNCH_CHECK("geglu_kernel");
    return 0;
}

int launch_timestep_embedding(const int64_t* t, bf16_t* out, int batch, int dim, hipStream_t stream) {
    if (dim % 2) return mkd_fail(-1, "timestep_embedding: odd dim");
    const int total = batch * (dim / 2);
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, t, out, batch, dim);
    MKD_LAUNCH_CHECK("timestep_embedding_kernel");
    return 0;
}

int launch_conv3x3_direct(const void* x, int in_nchw_f32, const bf16_t* w, const float* bias, void* y,
                          int out_nchw_f32, int act, const bf16_t* add, int batch, int Hin, int Win,
                          int Cin, int Cout, int stride, hipStream_t stream, const ConvInIo* second) {
    if (stride != 1 && stride != 2) return mkd_fail(-1, "conv3x3_direct: stride must be 1 or 2");
    // 4 -> C: the UNet / ControlNet input conv; 3 -> C: the VAE encoder's conv_in on the image (full resolution)
    if (in_nchw_f32 && !out_nchw_f32 && stride == 1 && ((Cin == 4 && Cout >= 64) || (Cin == 3 && Cout >= 8)) && Cout <= 512 && (Cin == 4 || !second)) {
        const int npix = batch * Hin * Win;
        const int ppb = 16;            // <= PPB_MAX of the kernel
        const int threads = (Cout + 63) / 64 * 64;
        Pair<ConvInIo> io;
        io.g[0] = ConvInIo{w, bias, (bf16_t*)y, add};
        MKD_PAIR_SET2(io, second ? *second : io.g[0]);
        if (Cin == 4)
            hipLaunchKernelGGL(conv3x3_fewin_kernel<4>, dim3((npix + ppb - 1) / ppb, second ? 2 : 1), dim3(threads), 0, stream, (const float*)x, io,
                               act, batch, Hin, Win, Cout, ppb);
        else
            hipLaunchKernelGGL(conv3x3_fewin_kernel<3>, dim3((npix + ppb - 1) / ppb, 1), dim3(threads), 0, stream, (const float*)x, io,
                               act, batch, Hin, Win, Cout, ppb);
        MKD_LAUNCH_CHECK("conv3x3_fewin_kernel");
        return 0;
    }
    if (second) return mkd_fail(-1, "conv3x3_direct: only the 4 -> C input convolution has a grouped form");
    if (!in_nchw_f32 && out_nchw_f32 && (Cout == 4 || Cout == 3) && stride == 1 && act == 0 && !add && Cin % 8 == 0) {
        const int npix = batch * Hin * Win;
        if (Cout == 4)
            hipLaunchKernelGGL(conv3x3_fewout_kernel<4>, dim3((npix + 3) / 4), dim3(256), 0, stream, (const bf16_t*)x, w, bias,
                               (float*)y, batch, Hin, Win, Cin);
        else
            hipLaunchKernelGGL(conv3x3_fewout_kernel<3>, dim3((npix + 3) / 4), dim3(256), 0, stream, (const bf16_t*)x, w, bias,
                               (float*)y, batch, Hin, Win, Cin);
        MKD_LAUNCH_CHECK("conv3x3_fewout_kernel");
        return 0;
    }
    const int Hout = (Hin + 2 - 3) / stride + 1, Wout = (Win + 2 - 3) / stride + 1;
    const int64_t total = (int64_t)batch * Hout * Wout * Cout;
    hipLaunchKernelGGL(conv3x3_direct_kernel, dim3(grid_for(total, 256, 1 << 20)), dim3(256), 0, stream, x, in_nchw_f32, w, bias,
                       y, out_nchw_f32, act, add, batch, Hin, Win, Cin, Cout, Hout, Wout, stride);
    MKD_LAUNCH_CHECK("conv3x3_direct_kernel");
    return 0;
}

int launch_vae_enc_tail(const bf16_t* x, const bf16_t* w, const float* bias, const bf16_t* wq, const float* bq, const float* noise,
                        float scale, float* z_out, float* moments_out, int batch, int H, int W, int Cin, int z_channels, hipStream_t stream) {
    if (z_channels != 4) return mkd_fail(-1, "vae_enc_tail: z_channels must be 4");
    if (Cin % 8 || !x || !w || !bias || !wq || !bq || (!z_out && !moments_out)) return mkd_fail(-1, "vae_enc_tail: bad arguments");
    const int npix = batch * H * W;
    hipLaunchKernelGGL(vae_enc_tail_kernel<4>, dim3((npix + 3) / 4), dim3(256), 0, stream, x, w, bias, wq, bq, noise, scale, z_out,
                       moments_out, batch, H, W, Cin);
    MKD_LAUNCH_CHECK("vae_enc_tail_kernel");
    return 0;
}

int launch_pack_conv_weight(const float* w, bf16_t* out, int Cout, int Cin, int kh, int kw, hipStream_t stream) {
    const int64_t total = (int64_t)Cout * Cin * kh * kw;
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3(grid_for(total, 256, 8192)), dim3(256), 0, stream, w, out, Cout, Cin, kh, kw);
    MKD_LAUNCH_CHECK("pack_conv_weight_kernel");
    return 0;
}

int launch_f32_to_bf16(const float* x, bf16_t* y, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, stream, x, y, n);
    MKD_LAUNCH_CHECK("f32_to_bf16_kernel");
    return 0;
}

int launch_bf16_to_f32(const bf16_t* x, float* y, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, stream, x, y, n);
    MKD_LAUNCH_CHECK("bf16_to_f32_kernel");
    return 0;
}

int launch_clip_embed(const int32_t* tokens, const bf16_t* tok_emb, const bf16_t* pos_emb, bf16_t* out, int batch, int T, int width,
                      int vocab, hipStream_t stream) {
    if (width % 8) return mkd_fail(-1, "clip_embed: width must be a multiple of 8");
    hipLaunchKernelGGL(clip_embed_kernel, dim3(grid_for((int64_t)batch * T * (width / 8))), dim3(256), 0, stream, tokens, tok_emb, pos_emb,
                       out, batch * T, T, width, vocab);
    MKD_LAUNCH_CHECK("clip_embed_kernel");
    return 0;
}

int launch_merge_ff_out(const float* P, const float* W2, const float* b2, const float* bp, bf16_t* Wm, float* bias_m, int d,
                        hipStream_t stream) {
    hipLaunchKernelGGL(merge_ff_out_kernel, dim3((5 * d + 255) / 256, d), dim3(256), 0, stream, P, W2, b2, bp, Wm, bias_m, d);
    MKD_LAUNCH_CHECK("merge_ff_out_kernel");
    return 0;
}

int launch_copy_strided(const bf16_t* src, int ld_src, bf16_t* dst, int ld_dst, int rows, int cols, hipStream_t stream) {
    if (cols % 8 || ld_src % 8 || ld_dst % 8) return mkd_fail(-1, "copy_strided: multiples of 8 required");
    hipLaunchKernelGGL(copy_strided_kernel, dim3(grid_for((int64_t)rows * (cols / 8))), dim3(256), 0, stream, src, ld_src, dst,
                       ld_dst, rows, cols);
    MKD_LAUNCH_CHECK("copy_strided_kernel");
    return 0;
}

int launch_repeat_batch(const float* x, float* y, int64_t n_per, int reps, hipStream_t stream) {
    hipLaunchKernelGGL(repeat_batch_kernel, dim3(grid_for(n_per * reps)), dim3(256), 0, stream, x, y, n_per, reps);
    MKD_LAUNCH_CHECK("repeat_batch_kernel");
    return 0;
}

int launch_fill_i64(int64_t* p, int64_t v, int n, hipStream_t stream) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, v, n);
    MKD_LAUNCH_CHECK("fill_i64_kernel");
    return 0;
}

static int temb_blocks(const TembSel& ts) {
    const long long v = ((long long)(ts.n[0] >> 2) + (ts.n[1] >> 2)) * ts.batch;
    long long b = (v + 1023) / 1024;          // ~4 float4 per thread
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}
int launch_temb_select(const TembSel& ts, int step, hipStream_t stream) {
    if ((ts.n[0] | ts.n[1]) & 3) return mkd_fail(-1, "temb_select: row lengths must be multiples of 4");
    if (!ts.n[0] && !ts.n[1]) return 0;
    hipLaunchKernelGGL(temb_select_kernel, dim3(temb_blocks(ts)), dim3(256), 0, stream, ts, step);
    MKD_LAUNCH_CHECK("temb_select_kernel");
    return 0;
}
int launch_step_setup(StepState* st, int64_t* t_out, int batch, float* x, int64_t n, hipStream_t stream, const TembSel* tsp) {
    TembSel ts; memset(&ts, 0, sizeof(ts));
    if (tsp) ts = *tsp;
    if ((ts.n[0] | ts.n[1]) & 3) return mkd_fail(-1, "step_setup: row lengths must be multiples of 4");
    if (!x || n <= 0) return mkd_fail(-1, "step_setup: no latent");
    int blocks = (ts.n[0] || ts.n[1]) ? temb_blocks(ts) : 1;
    // (the latent of a masked step: ~8 elements per thread; at the benchmark's shapes the time-embedding rows already need more)
    const int xb = grid_for((n + 7) / 8, 256, 512);
    if (xb > blocks) blocks = xb;
    hipLaunchKernelGGL(step_setup_kernel, dim3(blocks), dim3(256), 0, stream, st, t_out, batch, ts, x, n);
    MKD_LAUNCH_CHECK("step_setup_kernel");
    return 0;
}

int launch_cfg_rescale_factor(const float* eps_c, const float* eps_u, float cfg_scale, float phi, const StepState* st, int batch,
                              int n_per_sample, float* k_out, hipStream_t stream) {
    if (!eps_c || !eps_u || !k_out || batch <= 0 || n_per_sample <= 0) return mkd_fail(-1, "cfg_rescale_factor: bad arguments");
    hipLaunchKernelGGL(cfg_rescale_factor_kernel, dim3(batch), dim3(256), 0, stream, eps_c, eps_u, cfg_scale, phi, st, n_per_sample, k_out);
    MKD_LAUNCH_CHECK("cfg_rescale_factor_kernel");
    return 0;
}

// blocks along x for one sample of `per` elements: ~4 elements per thread (one 16-byte access), at most 64 per sample
static int rows_blocks(int per) {
    const int b = (per + 1023) / 1024;
    return b < 1 ? 1 : (b > 64 ? 64 : b);
}
int launch_step_setup_rows(StepState* st, int64_t* t_out, int batch, int samples, hipStream_t stream, const TembSel* tsp) {
    TembSel ts; memset(&ts, 0, sizeof(ts));
    if (tsp) ts = *tsp;
    if ((ts.n[0] | ts.n[1]) & 3) return mkd_fail(-1, "step_setup_rows: row lengths must be multiples of 4");
    if (!st || !t_out || samples <= 0 || batch <= 0 || batch > 65535 || batch % samples) return mkd_fail(-1, "step_setup_rows: bad arguments");
    if ((ts.n[0] || ts.n[1]) && ts.batch != batch) return mkd_fail(-1, "step_setup_rows: the time-embedding rows are not of this batch");
    const int nv = (ts.n[0] > ts.n[1] ? ts.n[0] : ts.n[1]) >> 2;
    int blocks = (nv + 1023) / 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(step_setup_rows_kernel, dim3(blocks, batch), dim3(256), 0, stream, st, t_out, samples, ts);
    MKD_LAUNCH_CHECK("step_setup_rows_kernel");
    return 0;
}

int check_rescale_args(const float* k, const float* eps_u, int64_t n, int n_per_sample, const char* who) {
    if (k && (!eps_u || n_per_sample <= 0 || n % n_per_sample))
        return mkd_fail(-1, std::string(who) + ": k needs eps_u and an n_per_sample > 0 that divides n");
    return 0;
}
// What the three step launchers share: the checks of the record's form and the launch.  missing: the record form (st null) lacks an
// operand that the solver's numbers need
template <class Kernel>
static int launch_step(Kernel kernel, const char* who, const StepOps& o, bool missing, hipStream_t stream) {
    const std::string w(who);
    if (!o.x || !o.eps_c || !o.x_out || o.n <= 0 || (o.st ? (o.x_out != o.x || o.rows) : missing)) return mkd_fail(-1, w + ": bad arguments");
    if (o.samples && (o.samples < 0 || o.samples > 65535 || o.per <= 0 || o.n != (int64_t)o.samples * o.per || o.kfac || (!o.st && !o.rows)))
        return mkd_fail(-1, w + ": bad arguments");
    if (int rc = check_rescale_args(o.kfac, o.eps_u, o.n, o.per, who)) return rc;
    const dim3 grid = o.samples ? dim3(rows_blocks(o.per), o.samples) : dim3(grid_for(o.n));
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, o);
    MKD_LAUNCH_CHECK(w + "_kernel");
    return 0;
}
int launch_ddim_step(const StepOps& o, hipStream_t stream) {
    if (o.n <= 0) return mkd_fail(-1, "ddim_step: empty");
    return launch_step(ddim_step_kernel, "ddim_step", o, false, stream);
}
int launch_dpmpp_step(const StepOps& o, hipStream_t stream) {
    const DpmCoef k = DpmCoef::from(o.coef);
    if (!o.st && !o.samples && ((k.c1 != 0.f && !o.hist[0]) || (k.c2 != 0.f && !o.hist[1])))
        return mkd_fail(-1, "dpmpp_step: a non-zero history coefficient needs its x0-prediction");
    return launch_step(dpmpp_step_kernel, "dpmpp_step", o, !o.p_out || (o.samples && (!o.hist[0] || !o.hist[1])), stream);
}
int launch_unipc_step(const StepOps& o, hipStream_t stream) {
    const UniCoef k = UniCoef::from(o.coef);
    const bool c = k.ac != 0.f;
    if (o.samples) return mkd_fail(-1, "unipc_step: no per-sample form");
    if (!o.st && ((c && !o.xc_prev) ||(((c && k.q1 != 0.f) || k.p1 != 0.f) && !o.hist[0]) ||
                  (((c && k.q2 != 0.f) || k.p2 != 0.f) && !o.hist[1]) || (c && k.q3 != 0.f && !o.hist[2])))
        return mkd_fail(-1, "unipc_step: a non-zero coefficient needs its corrected latent / x0-prediction");
    return launch_step(unipc_step_kernel, "unipc_step", o, !o.p_out || !o.xc_out, stream);
}

int launch_softmax_rows(const float* x, bf16_t* y, int rows, int cols, hipStream_t stream) {
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, stream, x, y, cols);
    MKD_LAUNCH_CHECK("softmax_rows_kernel");
    return 0;
}

int launch_post_quant(const float* z, const bf16_t* w, const float* bias, float inv_scale, float* out, int batch, int C, int hw,
                      hipStream_t stream) {
    hipLaunchKernelGGL(post_quant_kernel, dim3(grid_for((int64_t)batch * C * hw)), dim3(256), 0, stream, z, w, bias, inv_scale, out,
                       batch, C, hw);
    MKD_LAUNCH_CHECK("post_quant_kernel");
    return 0;
}

int launch_blend(const bf16_t* a, const bf16_t* b, const float* alpha, bf16_t* y, int64_t per_sample, int batch, hipStream_t stream) {
    if (per_sample % 8) return mkd_fail(-1, "blend: per-sample size must be a multiple of 8");
    hipLaunchKernelGGL(blend_kernel, dim3(grid_for(per_sample * batch / 8)), dim3(256), 0, stream, a, b, alpha, y, per_sample, batch);
    MKD_LAUNCH_CHECK("blend_kernel");
    return 0;
}

int launch_q_sample_blend(const float* x0, const float* noise, float sqrt_ac, float sqrt_1m_ac, const float* mask, int mask_batch,
                          int mask_channels, const float* x, float* out, int batch, int channels, int hw, hipStream_t stream) {
    if (!x0 || !noise || !out || batch <= 0 || channels <= 0 || hw <= 0) return mkd_fail(-1, "q_sample_blend: bad arguments");
    if (mask && (!x || (mask_batch != 1 && mask_batch != batch) || (mask_channels != 1 && mask_channels != channels)))
        return mkd_fail(-1, "q_sample_blend: mask must be [1 or B, 1 or C, h, w] and needs x");
    const int64_t n = (int64_t)batch * channels * hw;
    const int mcs = mask_channels == 1 ? 0 : hw;
    const int mbs = mask_batch == 1 ? 0 : mask_channels * hw;
    hipLaunchKernelGGL(q_sample_blend_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x0, noise, sqrt_ac, sqrt_1m_ac, mask, x, out, n, hw,
                       channels * hw, mbs, mcs);
    MKD_LAUNCH_CHECK("q_sample_blend_kernel");
    return 0;
}

int launch_latent_mask_from_labels(const uint8_t* labels, int batch, int H, int W, uint64_t classes, int f, float threshold, float* out,
                                   hipStream_t stream) {
    if (!labels || !out || batch <= 0 || f < 1 || f > 64 || H < f || W < f || H % f || W % f)
        return mkd_fail(-1, "latent_mask_from_labels: labels [B, H, W] with H, W multiples of the factor (1..64)");
    const int64_t total = (int64_t)batch * (H / f) * (W / f);
    hipLaunchKernelGGL(latent_mask_from_labels_kernel, dim3(grid_for(total)), dim3(256), 0, stream, labels, batch, H, W,
                       (unsigned long long)classes, f, threshold, out);
    MKD_LAUNCH_CHECK("latent_mask_from_labels_kernel");
    return 0;
}
