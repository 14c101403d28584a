// Shared declarations for libmkd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

typedef uint16_t bf16_t;   // raw bf16 bits on the host side of the launchers

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;

void mkd_set_error(const std::string& msg);
int mkd_fail(int code, const std::string& msg);

#define MKD_HIP_CHECK(expr)                                                            \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return mkd_fail(-2, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

#define MKD_LAUNCH_CHECK(what)                                                         \
    do {                                                                               \
        hipError_t _e = hipGetLastError();                                             \
        if (_e != hipSuccess)                                                          \
            return mkd_fail(-2, std::string(what) + ": " + hipGetErrorString(_e));     \
    } while (0)

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ float bf16_to_f32(uint16_t v) {
    return __uint_as_float(((uint32_t)v) << 16);
}
// round-to-nearest-even via the hardware convert (keeps NaN a NaN).
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}
// The 0..255 value and the bin of a [0, 1] pixel as mkd_hist_match and mkd_pgt_compose form them (NaN -> 0).  __fmul_rn: the product
// is rounded once whatever -ffp-contract says (it must not fuse into a following subtraction)
__device__ __forceinline__ float hm_value(float x) { return __fmul_rn(fminf(fmaxf(x, 0.0f), 1.0f), 255.0f); }
__device__ __forceinline__ int hm_bin(float v) { const int b = (int)v; return b > 255 ? 255 : b; }       // torch.histc(bins=256, min=0, max=256)
// Activation math on the hardware transcendental units (v_exp_f32 / v_rcp_f32, ~1 ulp each): an IEEE division costs ~10 VALU
// ops and libm erff ~40, and the element-wise kernels here are VALU-bound on the few CUs a GroupNorm can occupy.
__device__ __forceinline__ float sigmoid_scaled_f(float x, float k) {            // 1 / (1 + exp(-k x))
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * (-1.4426950408889634f * k)));
}
__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_scaled_f(x, 1.0f); }
__device__ __forceinline__ float quick_gelu_f(float x) { return x * sigmoid_scaled_f(x, 1.702f); }      // CLIP: x * sigmoid(1.702 x)
// erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, far below the bf16 output step): GELU(x) = x/2 * (1 + erf(x / sqrt 2))
__device__ __forceinline__ float gelu_erf_f(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
    float p = 1.061405429f;
    p = p * t - 1.453152027f;
    p = p * t + 1.421413741f;
    p = p * t - 0.284496736f;
    p = p * t + 0.254829592f;
    const float e = 1.0f - p * t * __builtin_amdgcn_exp2f(-1.4426950408889634f * z * z);      // erf(|x| / sqrt 2)
    return 0.5f * x * (1.0f + copysignf(e, x));
}

struct __attribute__((aligned(16))) U16x8 { uint16_t v[8]; };
struct __attribute__((aligned(8)))  U16x4 { uint16_t v[4]; };

// One correctly rounded product.  The __f*_rn forms are plain operators in HIP's headers and -ffp-contract=fast lets the backend fuse
// them all the same (p + q became fma(a, u, q)), so every product that feeds an addition goes through an empty asm statement first: no
// instruction, but the value is opaque and cannot become half of a fused multiply-add.
__device__ __forceinline__ float mkd_rounded(float x) {
    asm("" : "+v"(x));
    return x;
}
__device__ __forceinline__ double mkd_rounded(double x) {
    asm("" : "+v"(x));
    return x;
}
__device__ __forceinline__ double mkd_rounded_mul(double a, double b) { return mkd_rounded(a * b); }
#endif

// The checks every photo call makes on its HOST descriptor array (mkd_photo_desc or mkd_photo_frame_desc of include/mkd.h) -> the text
// of the first one that fails, else null: n and S, then per descriptor the photo fields, region(d) (the box's or the frame's own
// checks) and the label map that labels_out needs.
template <typename Desc, typename Region>
const char* mkd_check_photo_descs(const Desc* descs, int n, int S, bool need_labels, Region region) {
    if (!descs || n < 1 || n > 16) return "1..16 descriptors per call";          // MKD_PHOTO_MAX_BATCH
    if (S < 8 || S > 1024) return "S must be 8..1024";
    for (int i = 0; i < n; ++i) {
        const Desc& d = descs[i];
        if (!d.pixels) return "null pixels";
        if (d.H < 1 || d.W < 1 || d.H > 16384 || d.W > 16384) return "photo H, W must be 1..16384";
        if ((int64_t)d.pitch_bytes < (int64_t)3 * d.W) return "pitch_bytes must be >= 3 W";
        if (const char* e = region(d)) return e;
        if (need_labels && !d.labels) return "labels_out needs a label map in every descriptor";
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// kernel launch parameter blocks (host + device)
// ---------------------------------------------------------------------------------------------
struct GemmArgs {
    const bf16_t* A; int lda;
    const bf16_t* W; int ldw;
    const float* bias;
    const float* rowbias; int ldrb; int rows_per_batch;
    const bf16_t* R; int ldr;
    float scale; int act;
    void* C; int ldc; int out_f32;
    int M, N, K;
    int conv; int Hin, Win, Cin, Hout, Wout, stride, up;
    // conv: top/left padding of the 3x3 window (its origin is (oy * stride - pad_tl, ox * stride - pad_tl)).  1: pad 1 on every side,
    // the only form before the VAE encoder and what every conv builder sets; 0: UPSTREAM Downsample (F.pad(x, (0,1,0,1)) + a
    // stride-2 pad-0 conv), stride 2 without upsampling only, gather / linear and register-A kernels only (launch_gemm checks)
    int pad_tl;                             // (fills the 4-byte hole before ws: the block does not grow)
    float* ws; size_t ws_bytes; int splitk; int ksteps_per_split;     // split-K fp32 partial slabs: pointer and capacity
    int tile_h, tile_w, tile_imgs;          // spatial tile of the LDS-staged conv kernel (set by its launcher)
    const float* ln_s; float ln_eps;        // fused LayerNorm on the A rows: ln_s[n] = sum_k W'[n][k] (W' = W*gamma), else null
    const float* stat_in; int stat_in_slots; // ... whose row sums were emitted by the producer: [slots][M][2] (sum, sumsq)
    float* stat_out;                        // producer side: emit per-column-slot partial row sums of the (rounded) output
    // GroupNorm statistics of the tensor this GEMM writes (part of): gn_stat[sample][32][2] int64 fixed point (gemm_device.h);
    // gn_cg channels per group OF THE CONSUMER's tensor, gn_coff = column of this output inside it (concat halves), gn_hw rows per sample
    long long* gn_stat; int gn_cg; int gn_coff; int gn_hw;
    int defer_epilogue;                     // split-K launches: leave the fp32 partial slabs in ws; the caller's next kernel reduces them (launch_gn_from_slabs)
    int expect_splitk;                      // ... which was planned for exactly this many slabs: the launch fails if it resolves to another count (0: unchecked)
    // workgroup -> tile order for the 8 XCDs (workgroups are dealt round-robin to them in launch order, each XCD has its own L2):
    // 0 launch order; 1 an XCD owns runs of M-tiles of one N-tile (the weight tile lives in ONE L2); 2 runs of N-tiles of one M-tile
    int xcd_mode;
    int gz;               // z extent of ONE problem's grid (set by the launchers); a grouped launch stacks the second problem above it
    const bf16_t* zero;   // >= 16 bytes of zeros
    // conv3x3 with a folded 1x1 convolution of a SECOND input (ResBlock: out = conv3x3(h) + skip_connection(x), UPSTREAM ResBlock._forward):
    // K = 9 * Cin + K2, W = [W_conv | W_skip] (row-major over that K), the last K2 columns contract with row m of A2 ([M, K2] at lda2).
    // Gather / linear kernel only (stride 1, no upsampling); the tile plan is the one of the plain convolution (K - K2 in the tables)
    const bf16_t* A2; int lda2; int K2;
};

// ---------------------------------------------------------------------------------------------
// Grouped launches.  The ControlNet and the UNet encoder + middle block (reference diffmk/makeup_diffuse.py:164-168: the two
// calls of apply_model) run the SAME op sequence on identical shapes with different weights / inputs.  One launch can carry both
// problems: the kernel's argument block is a 2-entry table and a grid coordinate (z, or y for 1-D grids) selects the entry, so
// the pair costs ONE dependent dispatch instead of two on two contending queues.  Same kernels, same tiles, same order of
// operations per output: results are bit-identical to two separate launches.
// ---------------------------------------------------------------------------------------------
// MKD_PAIR_N = 1 (default build since round 4): single-entry argument tables.  The 2-entry form on every launch cost the DEFAULT
// two-chain plan 1.9 % (doubled kernarg blocks, a blockIdx.z-indexed indirection in every kernel: profiles/exp_r4_pair_form.txt,
// 5.39 vs 5.29 ms per evaluation, three alternating rounds), and its only user, the grouped encoder chain
// (MKD_ENC_GROUP, 10 % slower than two chains), is an experiment: build it with tools/build_variant.sh group -DMKD_PAIR_N=2.
#ifndef MKD_PAIR_N
#define MKD_PAIR_N 1
#endif
template <typename T> struct Pair { T g[MKD_PAIR_N]; };
#define MKD_PAIR_SET2(tab, val) do { if (MKD_PAIR_N > 1) (tab).g[MKD_PAIR_N - 1] = (val); } while (0)
typedef Pair<GemmArgs> GemmArgs2;
struct NormIo { const bf16_t* x; bf16_t* y; const float* gamma; const float* beta; };     // GroupNorm / LayerNorm operands of one problem
struct AttnIo { const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o; };
struct ConvInIo { const bf16_t* w; const float* bias; bf16_t* y; const bf16_t* add; };     // 4 -> C input convolution (same x for both nets)

// device-resident DDIM step state (hipGraph replay): tables of n_steps entries, counter runs n_steps-1 .. 0
#ifndef MKD_MAX_STEPS
#define MKD_MAX_STEPS 1024          // (include/mkd.h has the same definition)
#endif
// One entry of the per-sample step table (mkd_sample_rows): what sample b does in executed step k, at [k * batch + b] of a device
// buffer [S_max][batch] filled on the host per call.  64 bytes; the layout is mkd_step_row of include/mkd.h (engine.hip asserts it).
// A sample that has run all its steps keeps the timestep / table row of its entry 0 (the model is still evaluated for it) with active = 0
struct StepRow {
    int64_t t;
    float coef[4];          // sqrt(1/a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sqrt(1-a_t): StepState::coef of the sample's entry
    float sigma;
    float dpm[6];           // DpmCoef of the sample's entry (a DPM-Solver++ call)
    int temb_row;           // row of the call's time-embedding table that holds t
    int active;             // 0: the sample is finished, its rows are not touched
    float scale;            // the sample's guidance scale
};
struct StepState {
    int counter;
    int64_t timesteps[MKD_MAX_STEPS];
    float coef[4 * MKD_MAX_STEPS];         // DdimCoef of table entry i: sqrt(1/a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sqrt(1-a_t)
    // eta > 0 (cddim.py:74-78): x_prev += sigma_t * noise * temperature.  noise: [n_steps][n] fp32 on the device, row k = the draw of the
    // k-th EXECUTED step (index n_steps - 1 - k); null: deterministic loop
    float sigma[MKD_MAX_STEPS];
    const float* noise; float temperature; int n_steps;
    // The executed step k = n_steps - 1 - counter, published by the step's first kernel.  It is all the step's last kernel is told: that
    // kernel moves the counter (so it cannot read it) and looks table entry n_steps - 1 - k, the ring slots and the trace row up from k.
    int cur_row;
    // masked sampling (UPSTREAM DDIMSampler.ddim_sampling mask / x0): step_setup_kernel first blends the latent with q_sample(x0),
    // x <- (q[2i] x0 + q[2i+1] q_noise[row]) mask + (1 - mask) x, row = the executed step (n_steps - 1 - i).  x0 null: unmasked.
    // mask [mB, mC, h, w] is read at b * mask_bstride + c * mask_cstride + p (stride 0 broadcasts); q_hw = h * w, q_chw = C * h * w
    const float* x0; const float* mask; const float* q_noise;
    int mask_bstride, mask_cstride, q_hw, q_chw;
    float q[2 * MKD_MAX_STEPS];            // sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod of table entry i
    // DPM-Solver++ multistep loop (mkd_sample_dpmpp): x <- c_x x + c_0 m_k + c_1 m_{k-1} + c_2 m_{k-2}, m_k = (x - sigma_t e) / alpha_t the
    // x0-prediction of executed step k.  dpm[6 i ..] = 1/alpha_t, sigma_t, c_x, c_0, c_1, c_2 of table entry i (mkd_dpmpp_table);
    // ring [3][n] fp32 holds m_k in slot ring_slot(k, 0, 3).  ring null: a DDIM loop
    float dpm[6 * MKD_MAX_STEPS];
    float* ring;
    // UniPC predictor-corrector loop (mkd_sample_unipc): uni[12 i ..] = the row of table entry i (mkd_unipc_table); it shares `ring`,
    // here [4][n] with m_k in slot ring_slot(k, 0, 4), and carries the corrected latent x^c in xc [n].  xc null: not a UniPC loop
    float uni[12 * MKD_MAX_STEPS];
    float* xc;
    // intermediates trace (mkd_sample_extras): entry i is logged into row trace_row[i] (-1: not logged) of trace_x (the latent after the
    // step) and trace_x0 (the step's x0-prediction), each [rows][n] fp32 and each null when not asked for
    float* trace_x; float* trace_x0;
    short trace_row[MKD_MAX_STEPS];
    // guidance rescale (mkd_sample_extras.guidance_rescale): the phi cfg_rescale_factor_kernel reads inside a replayed step, so a new
    // phi needs no new capture
    float phi;
    // per-sample loop (mkd_sample_rows): rows [n_steps][rows_batch] on the device, n_steps = the longest sample's; the step's kernels
    // take timestep, coefficients, scale and sigma of sample b in executed step k = n_steps - 1 - counter from rows[k * rows_batch + b]
    // instead of the tables above.  null: the uniform loop
    const StepRow* rows; int rows_batch;
};
// The schedule-only numbers of one step, per solver, each built from its table row in ONE place.
// DDIM: sqrt(1/a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sqrt(1-a_t) (of_alphas: the expressions every table of them is filled with)
struct DdimCoef {
    float sqrt_at_inv, sqrt_aprev, dir_coef, s1m;
    __host__ __device__ static DdimCoef from(const float* c) { return {c[0], c[1], c[2], c[3]}; }
    static void of_alphas(float a_t, float a_prev, float sigma_t, float s1m, float* c) {
        c[0] = 1.0f / sqrtf(a_t); c[1] = sqrtf(a_prev); c[2] = sqrtf(1.0f - a_prev - sigma_t * sigma_t); c[3] = s1m;
    }
};
// DPM-Solver++: the six numbers of a mkd_dpmpp_table row
struct DpmCoef {
    float inv_alpha, sigma, cx, c0, c1, c2;
    __host__ __device__ static DpmCoef from(const float* c) { return {c[0], c[1], c[2], c[3], c[4], c[5]}; }
};
// UniPC: the first eleven of a mkd_unipc_table row (ac == 0: the step has no corrector)
struct UniCoef {
    float inv_alpha, sigma, ac, q0, q1, q2, q3, ap, p0, p1, p2;
    __host__ __device__ static UniCoef from(const float* c) { return {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10]}; }
};
// Ring slot of m_{k-j}, the x0-prediction of j executed steps before step k, in a ring of `depth` planes (m_k goes to slot k mod depth)
__host__ __device__ inline int ring_slot(int k, int j, int depth) { return (k + depth - j) % depth; }

// One step launch of any solver, passed to the kernel by value.  It says where the launch's numbers come from:
//   st null, samples 0   the record itself: coef and the pointers below (the exported stand-alone entries, the eager loop)
//   st non-null          the device step state at the executed step st->cur_row: table entry, noise row, ring slots, trace rows; in
//                        place (x_out == x); the step's LAST kernel, which moves the counter
//   samples > 0          one grid row per sample over its `per` elements, numbers and scale from the sample's StepRow (st->rows at the
//                        executed step, or `rows`); a finished sample's blocks return before any access
// x_prev / x_next = x_out may be x and xc_out may be xc_prev: element i is read before it is written.
struct StepOps {
    const float* x; const float* eps_c; const float* eps_u; float scale;      // e = eps_u + scale (eps_c - eps_u); eps_u null: eps_c
    const float* kfac;                     // non-null (needs eps_u): e is multiplied by kfac[i / per], the guidance-rescale factors
    int per, samples;                      // elements of one sample (kfac, rows); samples > 0: the per-sample grid
    int64_t n;                             // elements of the whole latent
    StepState* st; const StepRow* rows;
    float* x_out; float* p_out;            // the new latent; the x0-prediction (DDIM: or null; the solvers with a ring: m0_out)
    float* x_copy; float* p_copy;          // non-null: stored there once more (a trace row)
    float coef[12];                        // the solver's numbers: DdimCoef / DpmCoef / UniCoef::from
    float sigma, temperature; const float* noise;          // DDIM eta term: x_out += sigma noise temperature (noise null: none)
    const float* hist[3];                  // m_{k-1}, m_{k-2}, m_{k-3}: read only where a coefficient of theirs is non-zero
    const float* xc_prev; float* xc_out;   // UniPC: the corrected latent in (read only where a_c != 0) and out
};
// The rescale arguments of a step entry (who: the name its message starts with)
int check_rescale_args(const float* k, const float* eps_u, int64_t n, int n_per_sample, const char* who);

// Time embedding of a sampling call: row `step` of tab[k] ([steps, n[k]] fp32, one table per net) is copied into every one of
// the `batch` rows of proj[k] ([batch, n[k]]: what the ResBlock epilogues read as their per-sample row bias).  n[k] % 4 == 0; n[k] = 0: absent.
struct TembSel { const float* tab[2]; float* proj[2]; int n[2]; int batch; };

// launchers (each only enqueues on `stream`)
// picks tile + split-K (a.splitk==0: auto).  second != null: grouped launch of two problems of identical geometry (see Pair)
int  launch_gemm(GemmArgs a, hipStream_t stream, const GemmArgs* second = nullptr);
bool gemm_same_geometry(const GemmArgs& a, const GemmArgs& b);     // may the two run as one grouped launch?
int  gemm_pick_splitk(int M, int N, int K, int conv, int stride, int up);
bool gemm_cfg_folds_second_input(int cfg);     // may this tile configuration take GemmArgs::A2 (gather / linear kernel)?
int  gemm_resolve(const GemmArgs& a, int* cfg, int* splitk);       // the (tile, split-K) launch_gemm will use for exactly these arguments
int  gemm_stat_slots(int M, int N, int K);   // column slots a linear GEMM of this shape writes row statistics in
int  gemm_tile_index(int M, int N, int K, int conv, int stride, int up);   // index into the tile-configuration table (gemm_tiles.inc)
// one row of gemm_tiles.inc (the columns are described there)
enum TileFamily { TILE_GEMM, TILE_KSPLIT, TILE_LIGHT, TILE_PATCH, TILE_RA };
struct TileCfg { int index; const char* name; TileFamily family; int tm, tn, wm, wn, stages, kw, base; };
const TileCfg* gemm_tile_cfg(int cfg);       // null when cfg is not in the table
int  gemm_tile_info(int cfg, int* tile_m, int* tile_n, int* lds_staged_conv, const char** name);      // mkd_gemm_tile_info (include/mkd.h)
void gemm_set_xcd_mode(int mode);         // tests / experiments: 0 launch order, 1 / 2 contiguous runs per XCD (GemmArgs::xcd_mode)
void gemm_force_tile_cfg(int cfg);           // tuner/tests: force a tile config (-1 = heuristic)
void gemm_set_splitk_cap(int cap);
void gemm_set_override(int M, int N, int K, int conv, int stride, int up, int cfg, int splitk);   // in-eval tuner; M <= 0 clears all
int  gemm_plan_epoch();                       // bumped by every override change: launch plans re-build on the next mkd_prepare
int  gemm_num_tile_cfgs();
const char* gemm_tile_cfg_name(int cfg);
int  launch_splitk_epilogue(const GemmArgs& a, hipStream_t stream, const GemmArgs* second = nullptr);
bool conv_patch_supported(const GemmArgs& a, int cfg);
int  launch_conv_patch(GemmArgs a, int cfg, int splitk, hipStream_t stream, const GemmArgs* second = nullptr);
size_t gemm_ws_bytes(int M, int N, int splitk);

int launch_groupnorm(const bf16_t* x, int ld_in, const float* gamma, const float* beta, float eps, int silu,
                     bf16_t* y, int ld_out, int batch, int hw, int C, int groups, float* partials,
                     hipStream_t stream, const NormIo* second = nullptr,       // second: same geometry, grouped launch
                     int two_kernel_min_hw = 1 << 30);      // >= this many pixels per sample: the two full-chip launches (mkd_ctx::gn_2k_min_hw)
size_t groupnorm_partials_bytes(int batch, int hw, int groups);
int launch_gn_stats(const bf16_t* x, int ld_in, int batch, int hw, int C, int groups, float* partials, hipStream_t stream, int* nchunks_out);
// GroupNorm with producer-emitted statistics (gstat[batch][32][2] int64 fixed point, see gemm_device.h): element-wise apply,
// and the stand-alone producer of the same statistics for tensors whose writer cannot emit them
int launch_gn_apply_stats(const bf16_t* x, int ld_in, const float* gamma, const float* beta, float eps, int silu, bf16_t* y, int ld_out,
                          int batch, int hw, int C, const long long* gstat, hipStream_t stream);
// GroupNorm [+SiLU] of a split-K GEMM's output straight from its fp32 partial slabs (launched with defer_epilogue): one kernel
// does the slab reduction, the GEMM epilogue (bias, row bias, scale, residual, bf16 rounding) and the normalisation; the raw
// output is also stored when a.C is non-null.  a = the GEMM's arguments with ws / splitk as launch_gemm resolved them.
// Returns -4 when the geometry does not fit the single-pass kernel (the caller then runs the two kernels separately).
int launch_gn_from_slabs(const GemmArgs& a, const float* gamma, const float* beta, float eps, int silu, bf16_t* y, int ld_out,
                         int batch, int hw, hipStream_t stream, const GemmArgs* a2 = nullptr, const NormIo* second = nullptr);
bool gn_from_slabs_supported(int batch, int hw, int C);
int launch_gn_colstats(const bf16_t* x, int ld, int batch, int hw, int ncols, int cg, int coff, long long* gstat, hipStream_t stream);
int launch_fold_layernorm(const float* w, const float* gamma, const float* beta, const float* bias, int N, int K,
                          bf16_t* w_out, int dst_row0, int dst_row_mul, float* s_out, float* b_out, hipStream_t stream);
int launch_layernorm(const bf16_t* x, const float* gamma, const float* beta, float eps, bf16_t* y,
                     int rows, int d, hipStream_t stream, int ldx = 0, const NormIo* second = nullptr);      // ldx: input row stride (0 = d); y is dense
int launch_merge_ff_out(const float* P, const float* W2, const float* b2, const float* bp, bf16_t* Wm, float* bias_m, int d,
                        hipStream_t stream);
// ---- fused row-local transformer tail (kernels_tfm.hip) ----------------------------------------------------------------------
// The tensors the engine's unfused path uses, all device pointers: attn1.to_out [d][d] + bias; attn2.to_q folded with LayerNorm 2
// (W' = W diag(gamma), s = rowsum(W'), b' = W beta); attn2.to_out [d][d] + bias; the GEGLU projection folded with LayerNorm 3 with
// (value, gate) rows interleaved [8d][d] (+ s, b' in the same order); the merged [ff.net.2 . proj_out | proj_out] weight [d][5d] + bias.
struct TfmTailWeights {
    const bf16_t* w_o1; const float* b_o1;
    const bf16_t* w_q; const float* s_q; const float* b_q;
    const bf16_t* w_o2; const float* b_o2;
    const bf16_t* w_g; const float* s_g; const float* b_g;
    const bf16_t* w_m; const float* b_m;
};
// ---- fused head of a d = 320 SpatialTransformer (kernels_tfm.hip): GroupNorm apply (statistics from launch_gn_stats) + proj_in +
// LayerNorm 1 folded into the q | k | v projection, one launch per 64-token tile: h0 [M, d] and qkv [M, 3d] out
struct TfmHeadWeights {
    const float* gn_gamma; const float* gn_beta;
    const bf16_t* w_pi; const float* b_pi;                       // proj_in [d][d]
    const bf16_t* w_qkv; const float* s_qkv; const float* b_qkv; // [3d][d] folded with LayerNorm 1 (W' = W diag(gamma), s, b')
};
size_t tfm_head_weight_bytes(int d);
size_t tfm_head_vec_bytes(int d);
int tfm_head_pack_weights(int d, const TfmHeadWeights& src, bf16_t* wpk, float* vec, hipStream_t stream);       // synchronous
int launch_tfm_head(int d, const bf16_t* wpk, const float* vec, const bf16_t* x, int ldx, const float* gn_partials, int gn_chunks, float gn_eps,
                    bf16_t* h0, bf16_t* qkv, int M, int T, hipStream_t stream);
void   tfm_tail_set_trace(long long* buf);
bool   tfm_tail_supported(int d, int heads, int T, int Tk);      // T tokens per sample, Tk context keys
size_t tfm_tail_weight_bytes(int d);
size_t tfm_tail_vec_bytes(int d);
size_t tfm_tail_kv_bytes(int d, int batch);
double tfm_tail_flops(int d, int M, int Tk);
int tfm_tail_pack_weights(int d, const TfmTailWeights& src, bf16_t* wpk, float* vec, hipStream_t stream);       // synchronous
int launch_tfm_tail_pack_kv(int d, const bf16_t* kv, int ldkv, int batch, int Tk, bf16_t* out, hipStream_t stream);
int launch_tfm_tail(int d, const bf16_t* wpk, const float* vec, const bf16_t* a1, int lda, const bf16_t* h0, int ldh, const bf16_t* xin, int ldx,
                    const bf16_t* kvp, bf16_t* out, int ldo, int M, int T, int Tk, hipStream_t stream);
int launch_attention(const bf16_t* q, int ldq, const bf16_t* k, int ldk, const bf16_t* v, int ldv,
                     bf16_t* o, int ldo, int batch, int Tq, int Tk, int heads, int dh, float scale,
                     hipStream_t stream, int causal = 0, const AttnIo* second = nullptr);
int attn_set_trace(long long* buf);      // -DMKD_ATTN_TRACE builds: per-phase cycle sums of the attention kernel
int launch_geglu(const bf16_t* x, bf16_t* y, int rows, int inner, hipStream_t stream);
int launch_conv3x3_direct(const void* x, int in_nchw_f32, const bf16_t* w, const float* bias, void* y,
                          int out_nchw_f32, int act, const bf16_t* add, int batch, int Hin, int Win,
                          int Cin, int Cout, int stride, hipStream_t stream, const ConvInIo* second = nullptr);   // second: 4 -> C form only
int launch_pack_conv_weight(const float* w, bf16_t* out, int Cout, int Cin, int kh, int kw, hipStream_t stream);
// VAE encoder tail: conv_out (3x3, bf16 NHWC [B,H,W,Cin] -> 2 z_channels) + quant_conv + DiagonalGaussianDistribution sample / mode
// (noise [B,z,H,W] fp32 or null) x scale -> z_out [B,z,H,W] / moments_out [B,2z,H,W] fp32 NCHW (either may be null)
int launch_vae_enc_tail(const bf16_t* x, const bf16_t* w, const float* bias, const bf16_t* wq, const float* bq, const float* noise,
                        float scale, float* z_out, float* moments_out, int batch, int H, int W, int Cin, int z_channels, hipStream_t stream);
int launch_f32_to_bf16(const float* x, bf16_t* y, int64_t n, hipStream_t stream);
int launch_timestep_embedding(const int64_t* t, bf16_t* out, int batch, int dim, hipStream_t stream);
int launch_copy_strided(const bf16_t* src, int ld_src, bf16_t* dst, int ld_dst, int rows, int cols,
                        hipStream_t stream);
// The step updates (kernels_misc.hip), one kernel and one launcher per solver, every form of StepOps above.  Grid: grid_for(n), or
// (blocks of one sample, samples) for the per-sample forms.
// DDIM: p0 = (x - sqrt(1-a_t) e) / sqrt(a_t), x_out = sqrt(a_prev) p0 + sqrt(1-a_prev-sigma^2) e (+ sigma noise temperature)
int launch_ddim_step(const StepOps& o, hipStream_t stream);
// DPM-Solver++ multistep: p_out = m0 = (x - sigma e) / alpha, x_out = c_x x + c_0 m0 + c_1 hist[0] + c_2 hist[1]
int launch_dpmpp_step(const StepOps& o, hipStream_t stream);
// UniPC predictor-corrector, x = x~_k: p_out = m0 = (x - sigma e) / alpha; xc_out = a_c xc_prev + q_0 m0 + q_1 hist[0] + q_2 hist[1] + q_3 hist[2]
// (a_c == 0: xc_out = x); x_out = a_p xc_out + p_0 m0 + p_1 hist[0] + p_2 hist[1].  No per-sample form
int launch_unipc_step(const StepOps& o, hipStream_t stream);
// guidance rescale factor, one workgroup per sample: k[b] = phi std(eps_c[b]) / std(g[b]) + (1 - phi), g = fmaf(cfg_scale, eps_c - eps_u, eps_u)
// over the sample's n_per_sample elements; std(g) == 0: 1.  st non-null: phi is read from the step state (replayed steps).  fp64 sums in a
// fixed order: the bits depend on nothing but the inputs
int launch_cfg_rescale_factor(const float* eps_c, const float* eps_u, float cfg_scale, float phi, const StepState* st, int batch,
                              int n_per_sample, float* k_out, hipStream_t stream);
int launch_repeat_batch(const float* x, float* y, int64_t n_per, int reps, hipStream_t stream);
int launch_fill_i64(int64_t* p, int64_t v, int n, hipStream_t stream);
// first kernel of a replayed step: the timestep of step st->counter (+ the step's time-embedding rows when ts != null,
// + the masked-sampling blend of the latent x [n] when st->x0 != null; the grid always covers x, so one capture serves both).
// It publishes the executed step in st->cur_row.  The counter itself is advanced by the step's LAST kernel (the solver's step launch
// with st), so every workgroup here reads the same value.
int launch_step_setup(StepState* st, int64_t* t_out, int batch, float* x, int64_t n, hipStream_t stream, const TembSel* ts = nullptr);
// out = (sqrt_ac x0 + sqrt_1m_ac noise) mask + (1 - mask) x over [batch, channels, hw]; mask [mask_batch, mask_channels, hw] broadcast
// (mask_batch in {1, batch}, mask_channels in {1, channels}); mask null: out = the q_sample alone (x unused).  out may be x.
int launch_q_sample_blend(const float* x0, const float* noise, float sqrt_ac, float sqrt_1m_ac, const float* mask, int mask_batch,
                          int mask_channels, const float* x, float* out, int batch, int channels, int hw, hipStream_t stream);
// labels [batch, H, W] uint8 -> out [batch, 1, H/f, W/f]: the fraction of each f x f block whose label is in `classes` (bit l = label l);
// threshold > 0: 1 where that fraction >= threshold, else 0
int launch_latent_mask_from_labels(const uint8_t* labels, int batch, int H, int W, uint64_t classes, int f, float threshold, float* out,
                                   hipStream_t stream);
// ---- makeup score (kernels_hist.hip) --------------------------------------------------------------------------------------------
// labels [batch, H, W] uint8 -> mask [batch, H, W] uint8 (1 where the label is in `classes`) + count [batch].  box_classes != 0: only
// inside the bounding box of the box_classes labels grown by `margin` pixels per side and clipped to the image; box_out [batch, 4] =
// (row min, row max, col min, col max) of that box before growing, (INT_MAX, -1, INT_MAX, -1) when no pixel has such a label
int launch_region_mask_from_labels(const uint8_t* labels, int batch, int H, int W, uint64_t classes, uint64_t box_classes, int margin,
                                   uint8_t* mask_out, int32_t* count_out, int32_t* box_out, hipStream_t stream);
// n histogram-matching terms in at most five launches; index [n][4] (dst image, ref image, dst mask, ref mask) or null (term t uses t)
size_t hist_match_scratch_bytes(int n);
int hist_match_launches(int want_apply, int want_loss);
int launch_hist_match(const float* dst, const float* ref, const uint8_t* mask_dst, const uint8_t* mask_ref, const int32_t* index, int n, int H,
                      int W, float* matched, uint8_t* tables, float* loss, int32_t* counts, void* scratch, hipStream_t stream);
int launch_temb_select(const TembSel& ts, int step, hipStream_t stream);          // the same copy with a host-side step index (eager loop)
// ---- per-sample loop (kernels_misc.hip) ----
// first kernel of a per-sample step (st->rows non-null): t_out[b] = the timestep of sample b % samples in this executed step (`batch` rows:
// both halves with guidance), row temb_row of the tables into row b of each proj, and the executed step into st->cur_row
int launch_step_setup_rows(StepState* st, int64_t* t_out, int batch, int samples, hipStream_t stream, const TembSel* ts = nullptr);
int launch_softmax_rows(const float* x, bf16_t* y, int rows, int cols, hipStream_t stream);
int launch_post_quant(const float* z, const bf16_t* w, const float* bias, float inv_scale, float* out, int batch, int C, int hw,
                      hipStream_t stream);
int launch_clip_embed(const int32_t* tokens, const bf16_t* tok_emb, const bf16_t* pos_emb, bf16_t* out, int batch, int T, int width,
                      int vocab, hipStream_t stream);
int launch_bf16_to_f32(const bf16_t* x, float* y, int64_t n, hipStream_t stream);
int launch_blend(const bf16_t* a, const bf16_t* b, const float* alpha, bf16_t* y, int64_t per_sample, int batch, hipStream_t stream);
// ---- region-wise transfer from several references (kernels_region.hip) -----------------------------------------------------------
// out[b, p, :] = sum_r weights[b, r, p] * e[r][b, p, :] over R <= 8 bf16 NHWC embeddings (e: HOST array of R device pointers), fp32 in the
// order r = 0, 1, ... (product, then fused multiply-adds), one bf16 rounding; out may be e[0].  C % 8 == 0, 16-byte aligned pointers
int launch_region_blend(const bf16_t* const* e, const float* weights, bf16_t* out, int batch, int hw, int C, int R, hipStream_t stream);
// masks [K, B, H, W] uint8 (K = 1..7, a pixel belongs to the lowest k with a non-zero mask) -> out [B, K + 1, H/f, W/f] fp32: plane k + 1 =
// strength[b, k] (null: 1) x the owned fraction of the (2 feather + 1)^2 block window (clamped at the edges), plane 0 = max(0, 1 - the others)
int launch_region_weights(const uint8_t* masks, int n_masks, int batch, int H, int W, int f, int feather, const float* strength, float* out,
                          hipStream_t stream);
// pixel-space background paste after the decode: out = clamp((a (src + 1) / 2 + (1 - a) (image + 1) / 2) 2 - 1) over fp32 [batch, channels, H, W];
// a from labels [batch, f H, f W] (class fraction of the (2 feather + 1)^2 window of f x f blocks, clamped at the edges) or from mask
// [mask_batch, 1, H, W] as is (exactly one of the two); alpha_out [batch, 1, H, W] or null; out may be image.  One launch
int launch_paste_background(const float* image, const float* src, const uint8_t* labels, uint64_t classes, int f, int feather, const float* mask,
                            int mask_batch, float* out, float* alpha_out, int batch, int channels, int H, int W, hipStream_t stream);
