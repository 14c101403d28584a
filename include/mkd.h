/*
 * mkd.h — C ABI of libmkd.so: the MI355X (gfx950) DDIM-sampling hot path of MakeupDiffuse.
 *
 * The reference (jiean001/MakeupDiffuse) has NO C/FFI boundary: its hot path is Python
 * duck-typing over torch tensors.  Each entry point below names the
 * reference interface (file:line under /root/reference) whose arithmetic it replaces; the
 * Python binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - functions only ENQUEUE work on `stream` (no host sync) unless stated otherwise;
 *   - return 0 on success, <0 on error; mkd_last_error() gives the message (thread-local);
 *   - external layout is the reference's: NCHW fp32 latents/images, [B,77,C] fp32 context,
 *     int64 timesteps.  Internally activations are NHWC bf16, accumulation fp32.
 *   - no internal host threads; a context is not re-entrant (one stream at a time).
 *   - host synchronisation points (everything else only enqueues): mkd_ctx_create / mkd_weights_finalize / mkd_vae_finalize / mkd_clip_finalize
 *     and the first mkd_prepare of a new shape (plan building, hipDeviceSynchronize); mkd_sample(use_graph != 0), which waits on the host
 *     for the context's PREVIOUS graph-replayed loop before it rewrites the pinned step table (hipStreamSynchronize of the
 *     private loop stream) and then returns with the new loop enqueued (mkd_sample_rows likewise; with use_graph == 0 it also waits
 *     for `stream` up to the upload of its own step table); mkd_eps_profile (measures, so it waits); mkd_ctx_destroy.
 */
#ifndef MKD_H
#define MKD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mkd_ctx mkd_ctx;

/* yaml control_stage_config / unet_config (diffmodels/base_diffusion_makeup.yaml:52-84). */
typedef struct mkd_net_config {
    int32_t in_channels;            /* 4   */
    int32_t out_channels;           /* 4   */
    int32_t hint_channels;          /* 6   (src_img ‖ ref_img, makeup_diffuse.py:56) */
    int32_t model_channels;         /* 320 */
    int32_t num_res_blocks;         /* 2   */
    int32_t n_levels;               /* len(channel_mult) = 4 */
    int32_t channel_mult[8];        /* 1,2,4,4 */
    int32_t n_attention_resolutions;/* 3 */
    int32_t attention_resolutions[8];/* 4,2,1 */
    int32_t num_heads;              /* 8   */
    int32_t transformer_depth;      /* 1 (only 1 is supported) */
    int32_t context_dim;            /* 768 */
    int32_t hint_widths[7];         /* 16,16,32,32,96,96,256 (cldm input_hint_block) */
} mkd_net_config;

#define MKD_OK              0
#define MKD_ERR_ARG        -1
#define MKD_ERR_HIP        -2
#define MKD_ERR_STATE      -3
#define MKD_ERR_UNSUPPORTED -4
#define MKD_ERR_MISSING    -5

const char* mkd_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int mkd_abi_version(void);
/* 1 when the library was built with 2-entry kernel argument tables (-DMKD_PAIR_N=2): the grouped encoder chain experiment
 * (MKD_ENC_GROUP=1) is available; the default build has single-entry tables (1.9 % faster on the default plan) and refuses it. */
int mkd_grouped_launches_available(void);

/* ---- context ---------------------------------------------------------------------------- */
/* Replaces cldm.model.create_model(yaml) for the two nets (runs/test.py:27). */
int  mkd_ctx_create(const mkd_net_config* cfg, mkd_ctx** out);
void mkd_ctx_destroy(mkd_ctx* ctx);

/* Replaces model.load_state_dict (runs/test.py:59-60) for keys under
 * "model.diffusion_model." and "control_model." (upstream names).
 * `data` is fp32, host OR device, `shape` is host. Synchronous. Unknown names -> MKD_ERR_ARG.
 * Loading a net weight invalidates the prepared conditioning: mkd_eps / mkd_sample fail (MKD_ERR_STATE) until mkd_weights_finalize +
 * mkd_prepare ran again; the weight forms mkd_weights_finalize derives are rebuilt and their previous generation is freed. */
int mkd_load_weight(mkd_ctx* ctx, const char* name, const float* data, int ndim, const int64_t* shape);
/* Checks every expected tensor was loaded, builds fused/packed weights. Synchronous. */
int mkd_weights_finalize(mkd_ctx* ctx);
/* Number of parameters expected (for the 859.5 M / 361.3 M check); which: 0 unet, 1 control, 2 first-stage decoder,
 * 3 text encoder, 4 first-stage encoder. */
int64_t mkd_param_count(const mkd_ctx* ctx, int which);
/* Enumerate the expected state_dict entries (sorted by name): count, name, shape (returns ndim <= 4). */
int mkd_param_total(const mkd_ctx* ctx);
const char* mkd_param_name(const mkd_ctx* ctx, int index);
int mkd_param_shape(const mkd_ctx* ctx, int index, int64_t* shape4);

/* Per-context plan switches (round 4: what used to be read from MKD_* environment variables once per process; the variables still
 * give the initial values).  Takes effect at the next mkd_prepare (the launch plan is re-built).  Names:
 *   "tfm_tail"             fused row-local transformer tail: 0 off, 1 wherever the kernel covers the shape, -1 shape policy (default)
 *   "tfm_tail_min_rows"    ... the policy's threshold on the rows (samples x tokens) of a block (default 4096)
 *   "skip_fold"            ... ResBlocks with a 1x1 skip_connection: conv2 and the skip as one implicit GEMM (K = 9 Cout + Cin) where
 *                          conv2's plan is the gather kernel: 0 off, 1 on (default)
 *   "tfm_head"             ... and the block's head (GroupNorm apply + proj_in + LayerNorm 1 . q|k|v) as one launch behind a GroupNorm
 *                          statistics launch wherever the tail is fused: 0 off, 1 on (default)
 *   "gn_2k_min_hw"         GroupNorm over >= this many pixels per sample: two full-chip launches (default 4096)
 *   "xcd_auto_ratio"       XCD-aware tile order where M <= ratio x N (default 1; 0 = launch order everywhere)
 *   "dec_lanes"            decoder batch lanes 0 / 2 / 4 (default 2)
 *   "ln_fly"               bit mask: LayerNorm taken on the fly by 1 = q|k|v, 2 = attn2.to_q, 4 = GEGLU projection (default 2)
 *   "gn_slab_min_channels" slab-fed GroupNorm from this many channels (default 1280)
 *   "graph_steps"          DDIM steps per captured graph (default 5)
 * Unknown names return MKD_ERR_ARG.  The tile tuner's state (mkd_gemm_force_tile / _set_xcd_mode / _set_override) stays process-global
 * by design (single-kernel entries, tuners): a change makes EVERY live context re-plan at its next mkd_prepare; mkd_live_contexts()
 * says how many there are. */
int mkd_ctx_set_option(mkd_ctx* ctx, const char* name, double value);
int mkd_ctx_get_option(const mkd_ctx* ctx, const char* name, double* value);
int mkd_live_contexts(void);

/* ---- conditioning ----------------------------------------------------------------------- */
/* Binds the step-invariant conditioning for a batch (cond dict of makeup_diffuse.py:42-57,
 * 152-166): hint = cat(c_concat,1) [B,hint_channels,8h,8w] in [0,1]; context = cat(c_crossattn,1)
 * [B,77,context_dim]; control_scales host [13] (makeup_diffuse.py:166) or NULL for all-ones;
 * only_mid_control (makeup_diffuse.py:162,168).  hint == NULL selects the `c_concat is None`
 * branch (makeup_diffuse.py:160-162).  Computes and caches the ControlNet hint embedding and
 * every cross-attention K/V projection (both independent of x and t).  (Re)allocates the
 * workspace when batch/h/w change (the only place that allocates). */
int mkd_prepare(mkd_ctx* ctx, int batch, int h, int w, const float* hint, const float* context,
                const float* control_scales, int only_mid_control, void* stream);

/* Makeup INTERPOLATION between two references (BUILD-DEFINED: the reference only shows a figure, README.md:23-25; SURVEY.md
 * §8f rank 2): like mkd_prepare, but the cached ControlNet hint embedding is the per-sample blend
 * (1 - alpha[b]) * E(hint_a[b]) + alpha[b] * E(hint_b[b]); hint_a = src||ref1, hint_b = src||ref2, alpha device fp32 [B]. */
int mkd_prepare_interp(mkd_ctx* ctx, int batch, int h, int w, const float* hint_a, const float* hint_b, const float* alpha,
                       const float* context, const float* control_scales, int only_mid_control, void* stream);

/* Region-wise makeup transfer from SEVERAL references (BUILD-DEFINED like interpolation, DESIGN.md §0: lips from one reference, eye
 * shadow from another, skin from a third, each with its own strength).  Like mkd_prepare, but the cached ControlNet hint embedding is
 * the spatial blend  E[b,y,x,:] = sum_r weights[b,r,y,x] * E(hints[r])[b,y,x,:]  of n_hints = R (1..8) embeddings, hints[r] = src||ref_r,
 * index 0 the base (src||src as hint 0 fades towards "no makeup").  hints: HOST array of R device pointers, each [B,hint_channels,8h,8w];
 * weights: DEVICE fp32 [B,R,h,w], arbitrary values (mkd_region_weights builds them from region masks), read when the call runs: new
 * weights with the same R do not re-plan.  The sum is fp32 in the order r = 0, 1, ... (w0 e0, then fma(w_r, e_r, acc)), rounded to bf16
 * once.  Costs R - 1 hint-block passes and one launch more than mkd_prepare, and nothing per step: guidance (prepare 2B with hints and
 * weights doubled), masked sampling, inversion and the DPM-Solver++ loop start from the prepared conditioning unchanged.
 * n_hints outside 1..8, a null pointer or a bad shape: MKD_ERR_ARG before anything is enqueued. */
int mkd_prepare_regions(mkd_ctx* ctx, int batch, int h, int w, const float* const* hints, int n_hints, const float* weights,
                        const float* context, const float* control_scales, int only_mid_control, void* stream);
/* Blend weights from region masks.  masks uint8 [n_masks][batch][H][W] (n_masks = K = R - 1 in 1..7, non-zero = inside; the layout of
 * mkd_region_mask_from_labels outputs stacked region-major), factor f in 1..64 with H, W multiples of it, feather rho in 0..4 latent
 * pixels, strength DEVICE fp32 [batch][K] or NULL (all ones) -> out [batch][K+1][H/f][W/f] fp32:
 *   a pixel belongs to the LOWEST k whose mask is non-zero (priority resolves overlaps), else to nobody;
 *   cnt_k(y,x) = owned pixels of latent block (y,x); S_k = sum of cnt_k over the (2 rho + 1)^2 window, indices clamped to the edge;
 *   a_k = float(S_k) / float((2 rho + 1)^2 f^2);  w_{k+1} = strength[b,k] * a_k;  w_0 = max(0, ((1 - w_1) - w_2) - ...), fp32 in that order.
 * Integer counts and one correctly rounded operation per step: the output has the bits of a numpy float32 restatement.  One launch,
 * the block counts of a sample staged in LDS (K * (H/f) * (W/f) <= 32768, else MKD_ERR_ARG); no scratch, no atomics, no host sync.
 * Bad shapes, n_masks outside 1..7, a null masks / out or feather outside 0..4: MKD_ERR_ARG before anything is enqueued. */
int mkd_region_weights(const uint8_t* masks, int n_masks, int batch, int H, int W, int factor, int feather, const float* strength,
                       float* out, void* stream);
/* The blend of mkd_prepare_regions as a stand-alone kernel (unit tests): e_ptrs HOST array of R (1..8) device pointers to bf16 NHWC
 * [batch, hw, C] embeddings (16-byte aligned, C a multiple of 8), weights fp32 [batch, R, hw], out bf16 [batch, hw, C]; out may alias
 * e_ptrs[0].  MKD_ERR_ARG as above. */
int mkd_region_blend_bf16(const uint16_t* const* e_ptrs, const float* weights, uint16_t* out, int batch, int hw, int C, int R, void* stream);
/* Tests only, like mkd_debug_poison: copies the cached ControlNet hint embedding [B,h,w,model_channels] bf16 out (enqueued on `stream`).
 * MKD_ERR_STATE when no conditioning with a hint is prepared. */
int mkd_debug_hint_embedding(mkd_ctx* ctx, uint16_t* out_bf16, void* stream);
/* Tests only: the first-stage mid-block attention (GroupNorm -> q|k, V^T -> fp32 scores -> softmax -> P.V + bv -> proj_out + x) alone,
 * of the decoder (which = 2) or the encoder (which = 4) of `ctx`, with the weights of that finalised network.  It emits and runs the
 * same op sequence the decode / encode plans hold.  x, out bf16 NHWC [batch, H, W, C] (out must not alias x); o bf16 [batch*H*W, C]
 * (may be NULL) receives the attention output before proj_out.  C must be the network's mid width ch * ch_mult[last] and H * W a
 * multiple of 8.  The plan and the workspace of the call are its own and are released before it returns (it synchronises `stream`): a
 * later mkd_decode / mkd_encode gives the bits it gave before.  MKD_ERR_STATE when that network is not finalised; MKD_ERR_ARG for
 * a null ctx / x / out, a bad shape, another `which`, or C != mid width. */
int mkd_debug_vae_attn(mkd_ctx* ctx, int which, const uint16_t* x_bf16_nhwc, int batch, int H, int W, int C, uint16_t* out_bf16,
                       uint16_t* o_bf16, void* stream);

/* ---- one eps evaluation ----------------------------------------------------------------- */
/* Replaces apply_model (makeup_diffuse.py:152-170): ControlNet -> 13 residuals x scale ->
 * ControlledUnet.  x [B,4,h,w] fp32 NCHW, t [B] int64 (device), eps_out [B,4,h,w] fp32. */
int mkd_eps(mkd_ctx* ctx, const float* x, const int64_t* t, float* eps_out, void* stream);

/* ---- DDIM update ------------------------------------------------------------------------ */
/* Replaces cddim.py:39-40 (CFG combine, eps_u may be NULL) and :56-78 (x0 / x_{t-1}).
 * All tensors have n elements; noise may be NULL (sigma_t == 0); pred_x0 may be NULL. */
int mkd_ddim_step(const float* x, const float* eps_c, const float* eps_u, float cfg_scale,
                  float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at,
                  const float* noise, float temperature,
                  float* x_prev, float* pred_x0, int64_t n, void* stream);

/* ---- guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4; rescale_noise_cfg
 * of published samplers).  BUILD-DEFINED on eps: with g = eps_u + scale (eps_c - eps_u), per sample b over its
 * n_per_sample elements  k[b] = phi std(eps_c[b]) / std(g[b]) + (1 - phi)  and the step uses e = g k[b]; std(g[b]) == 0 gives k[b] = 1.
 * mkd_cfg_rescale_factor: eps_c, eps_u [batch][n_per_sample] fp32 -> k_out [batch] fp32.  One launch, one workgroup per sample;
 * g = fmaf(scale, eps_c - eps_u, eps_u) in fp32, the sums of eps_c, eps_c^2, g, g^2 in fp64 in a fixed order (the same bits on every
 * run, for every batch), k in double, rounded once; a variance of g not above the rounding error of its own sums
 * (4 n_per_sample 2^-52 sum g^2) counts as zero.  No context, no atomics, no scratch, no host sync.
 * phi outside [0, 1], batch outside 1..65535, n_per_sample < 1, a null pointer: MKD_ERR_ARG. */
int mkd_cfg_rescale_factor(const float* eps_c, const float* eps_u, float scale, float phi, int batch, int n_per_sample,
                           float* k_out, void* stream);
/* mkd_ddim_step with the rescaled eps: k non-null (device [n / n_per_sample], needs eps_u and n_per_sample > 0 dividing n, else
 * MKD_ERR_ARG): e = fmaf(cfg_scale, eps_c - eps_u, eps_u) * k[i / n_per_sample], the expression the in-library loop uses.
 * k == NULL is exactly mkd_ddim_step. */
int mkd_ddim_step_ex(const float* x, const float* eps_c, const float* eps_u, float cfg_scale,
                     float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at,
                     const float* noise, float temperature, const float* k, int n_per_sample,
                     float* x_prev, float* pred_x0, int64_t n, void* stream);

/* ---- whole reverse loop ------------------------------------------------------------------ */
/* Replaces MKDDIMSampler.reconstruct (cddim.py:81-100) / DDIMSampler.ddim_sampling reached from
 * sample_log (diffusion_makeup.py:393-408) for eta == 0.  The context must have been prepared with
 * batch B (cfg_scale == 1) or 2B with the UNCONDITIONAL conditioning first (cddim.py:25-31).
 * Tables are host arrays of length n_steps indexed like ddim_alphas[index]; the loop runs
 * index = n_steps-1 .. 0 with timestep = timesteps[index].  x_T, x_out: [B,4,h,w] fp32.
 * use_graph != 0 captures one step into a hipGraph and replays it; such a call first waits (host) until the previous
 * graph-replayed loop of this context has finished, see "host synchronisation points" above.
 * DDIM inversion (UPSTREAM DDIMSampler.encode, eta 0) is the same update with a_t := ddim_alphas_prev[i] and
 * a_prev := ddim_alphas[i], executed in increasing i: pass MIRRORED tables, entry j = inversion step t_enc-1-j with
 * timesteps = ddim_timesteps, alphas = ddim_alphas_prev, alphas_prev = ddim_alphas, sqrt_one_minus = sqrt(1 - ddim_alphas_prev)
 * (makeupdiffuse_amd/ddim.py DDIMSampler.encode is the one place that builds them). */
int mkd_sample(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps,
               const float* alphas, const float* alphas_prev, const float* sqrt_one_minus_alphas,
               float cfg_scale, float* x_out, int use_graph, void* stream);

/* The same loop with eta > 0 (cddim.py:56-78 / UPSTREAM DDIMSampler.p_sample_ddim: dir_xt = sqrt(1 - a_prev - sigma_t^2) e_t,
 * x_prev += sigma_t * noise * temperature).  sigmas: host array like the other tables (ddim_sigmas[index]); noise: DEVICE array
 * [n_steps][B*4*h*w] fp32, row k = the draw of the k-th executed step (the caller draws them in loop order, as the reference's
 * noise_like does step by step); both NULL, or every sigma 0: mkd_sample.  The graph replays unchanged (the step reads its
 * sigma / noise row from the device-resident step state).  `noise` is read by the enqueued loop: it must stay valid until the work
 * on `stream` has completed. */
int mkd_sample_eta(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps,
                   const float* alphas, const float* alphas_prev, const float* sqrt_one_minus_alphas,
                   const float* sigmas, const float* noise, float temperature,
                   float cfg_scale, float* x_out, int use_graph, void* stream);

/* ---- masked sampling: background-preserving transfer (UPSTREAM DDIMSampler.ddim_sampling mask / x0) ------------------ */
/* Before every executed step (index i, timestep ts = timesteps[i]; before the model is evaluated) the latent is blended with a
 * forward-diffused x0:  img = (sqrt_alphas_cumprod[i] x0 + sqrt_one_minus_alphas_cumprod[i] n_k) mask + (1 - mask) img,
 * mask = 1 keeps x0.  There is no blend after the last step.  The tables are host arrays indexed like ddim_alphas[index], holding
 * the DDPM schedule's values at the step's timestep (model.sqrt_alphas_cumprod[ts]).  x0 [B,4,h,w] fp32 device: the un-doubled
 * batch, also with guidance; mask [mask_batch, mask_channels, h, w] fp32 device, mask_batch in {1, B}, mask_channels in {1, 4},
 * broadcast.  noise: DEVICE array [n_steps][B*4*h*w], row k = the blend's draw of the k-th executed step (upstream q_sample's
 * randn_like(x0); a caller that also passes eta > 0 noise draws the blend's row before the step's eta draw). */
typedef struct mkd_sample_mask {
    const float* x0;
    const float* mask;
    int32_t mask_batch;
    int32_t mask_channels;
    const float* sqrt_alphas_cumprod;              /* host [n_steps] */
    const float* sqrt_one_minus_alphas_cumprod;    /* host [n_steps] */
    const float* noise;                            /* device [n_steps][B*4*h*w] */
} mkd_sample_mask;
/* mkd_sample_eta with the blend above; m == NULL is exactly mkd_sample_eta.  All three loop forms (graph replay, its per-stream
 * segments, use_graph == 0) run it, with or without guidance, eta > 0 included.  The graph replays unchanged: its first kernel
 * reads x0 / mask / the noise row / the coefficients from the device-resident step state, so masked and unmasked calls share one
 * capture and the per-step launch count (mkd_step_launches) is the same; the eager loop (use_graph == 0) adds one launch per
 * step.  Bad shapes or a missing pointer in `m`: MKD_ERR_ARG.  x0, mask and noise are read by the enqueued loop: they must stay
 * valid until the work on `stream` has completed. */
int mkd_sample_masked(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps,
                      const float* alphas, const float* alphas_prev, const float* sqrt_one_minus_alphas,
                      const float* sigmas, const float* noise, float temperature, const mkd_sample_mask* m,
                      float cfg_scale, float* x_out, int use_graph, void* stream);
/* ---- extras of the in-library loop: the sampler's intermediates and guidance rescale -------------------------------------------
 * Trace (UPSTREAM DDIMSampler.ddim_sampling's intermediates): executed step k = 0 .. n_steps-1 runs table entry i = n_steps-1-k; entry i
 * is logged when i % log_every_t == 0 or i == n_steps-1; logged steps fill rows 0, 1, ... in execution order.  Row r of trace_x is the
 * latent after that step (masked sampling: before the next step's blend), row r of trace_x0 the step's x0-prediction
 * ((x - sqrt(1 - a_t) e) / sqrt(a_t) for DDIM, m_k for DPM-Solver++; e is the eps the update itself uses, guided and rescaled).
 * trace_x / trace_x0: DEVICE [rows][B*4*h*w] fp32, each may be NULL (that list is not kept); with either, rows must equal
 * mkd_sample_log_rows(n_steps, log_every_t) and log_every_t >= 1, else MKD_ERR_ARG.  The rows are written by the step's last kernel
 * (no extra launch; traced and untraced calls share one capture).  They are WRITTEN by the enqueued loop: they must stay valid until
 * the work on `stream` has completed, like `noise` of mkd_sample_eta.
 * guidance_rescale = phi in [0, 1] (else MKD_ERR_ARG): see mkd_cfg_rescale_factor; per sample, inside every step.  Engaged only with
 * guidance (cfg_scale != 1) and phi > 0: one extra launch per step (mkd_step_launches_ex cfg_on = 2), captured steps are keyed on it,
 * phi itself is read from the device-resident step state (a new phi does not re-capture).  phi = 0 or cfg_scale == 1: today's step. */
typedef struct mkd_sample_extras {
    int32_t log_every_t;
    int32_t rows;
    float*  trace_x;              /* device [rows][B*4*h*w] or NULL */
    float*  trace_x0;             /* device [rows][B*4*h*w] or NULL */
    float   guidance_rescale;     /* phi */
} mkd_sample_extras;
/* HOST only: the number of rows the rule above logs; n_steps < 1 or log_every_t < 1: MKD_ERR_ARG. */
int mkd_sample_log_rows(int n_steps, int log_every_t);
/* mkd_sample_masked with the extras; ex == NULL is exactly mkd_sample_masked (m == NULL as there).  All three loop forms. */
int mkd_sample_masked_ex(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps,
                         const float* alphas, const float* alphas_prev, const float* sqrt_one_minus_alphas,
                         const float* sigmas, const float* noise, float temperature, const mkd_sample_mask* m,
                         const mkd_sample_extras* ex, float cfg_scale, float* x_out, int use_graph, void* stream);
/* One blend / q_sample (the eager step loop's and DDIMSampler.stochastic_encode's kernel; the same device arithmetic as the loop):
 * out = (sqrt_ac x0 + sqrt_one_minus_ac noise) mask + (1 - mask) x over [batch, channels, hw] fp32 device tensors, mask as in
 * mkd_sample_mask (mask_batch in {1, batch}, mask_channels in {1, channels}); mask == NULL: out = the q_sample alone (x unused).
 * out may alias x.  Bad shapes: MKD_ERR_ARG. */
int mkd_q_sample_blend(const float* x0, const float* noise, float sqrt_ac, float sqrt_one_minus_ac, const float* mask,
                       int mask_batch, int mask_channels, const float* x, float* out, int batch, int channels, int hw, void* stream);
/* ---- DPM-Solver++ multistep sampler (Lu et al. 2022, Algorithm 2; UPSTREAM ldm.models.diffusion.dpm_solver, data prediction) ---- */
/* Deterministic, eps parameterisation, on the step grid and tables of DDIMSampler.make_schedule: table entry i goes from
 * a_t = alphas[i] to a_prev = alphas_prev[i] with the model evaluated at the integer timesteps[i]; the loop runs i = n_steps-1 .. 0
 * (upstream's wrapper evaluates at fractional timesteps of a continuous schedule; the engine's are int64, that form is not built).
 * With alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), h = lambda(a_prev) - lambda(a_t) and m_k = (x - sigma_t e) / alpha_t
 * the x0-prediction of executed step k, every step is  x <- c_x x + c_0 m_k + c_1 m_{k-1} + c_2 m_{k-2}:
 *   order 1: x <- (sigma_prev / sigma_t) x - alpha_prev expm1(-h) m_k        (algebraically the eta = 0 DDIM step)
 *   order 2: the same with D = (1 + 1/(2r)) m_k - 1/(2r) m_{k-1} for m_k, r = (lambda_t - lambda of the previous evaluation) / h
 *   order 3: multistep_dpm_solver_third_update (phi_1 = expm1(-h), phi_2 = phi_1 / h + 1, phi_3 = phi_2 / h - 1/2)
 * Executed step k uses order min(order, k + 1), and with lower_order_final != 0 and n_steps < 10 also at most n_steps - k.
 *
 * mkd_dpmpp_table: HOST only (no device, no context).  out [n_steps][6] = 1/alpha_t, sigma_t, c_x, c_0, c_1, c_2 of table entry i, computed in
 * double and stored as float; step_order [n_steps] (may be NULL) = the order entry i runs at.  MKD_ERR_ARG: order outside 1..3, an alpha
 * outside (0, 1), lambda not increasing along the executed steps. */
int mkd_dpmpp_table(int n_steps, const float* alphas, const float* alphas_prev, int order, int lower_order_final, float* out,
                    int* step_order);
/* One update: e = eps_u + cfg_scale (eps_c - eps_u) (eps_u NULL: eps_c); m0_out = (x - coef6[1] e) coef6[0];
 * x_prev = coef6[2] x + coef6[3] m0 + coef6[4] m1 + coef6[5] m2.  coef6: HOST, one row of mkd_dpmpp_table; m1 / m2 (the previous two
 * x0-predictions) are read only where their coefficient is non-zero and may be NULL otherwise; x_prev may alias x.  All fp32 [n]. */
int mkd_dpmpp_step(const float* x, const float* eps_c, const float* eps_u, float cfg_scale, const float* coef6, const float* m1,
                   const float* m2, float* x_prev, float* m0_out, int64_t n, void* stream);
/* ... with the rescaled eps: k / n_per_sample as in mkd_ddim_step_ex; k == NULL is exactly mkd_dpmpp_step. */
int mkd_dpmpp_step_ex(const float* x, const float* eps_c, const float* eps_u, float cfg_scale, const float* coef6, const float* m1,
                      const float* m2, const float* k, int n_per_sample, float* x_prev, float* m0_out, int64_t n, void* stream);
/* The whole loop: mkd_sample's contract (prepared batch B or 2B with the unconditional conditioning first, host tables, all three
 * loop forms: graph replay, its per-stream segments, use_graph == 0) with the update above as the step's last kernel and a device
 * history ring [3][B*4*h*w] fp32 owned by the context.  m != NULL: the masked blend of mkd_sample_masked before every step.  The
 * per-step launch count equals mkd_step_launches_ex.  Captured steps are keyed on the solver, so DDIM and DPM calls may alternate. */
int mkd_sample_dpmpp(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps, const float* alphas,
                     const float* alphas_prev, int order, int lower_order_final, const mkd_sample_mask* m, float cfg_scale,
                     float* x_out, int use_graph, void* stream);
/* mkd_sample_dpmpp with the extras of mkd_sample_masked_ex (trace_x0 rows are m_k); ex == NULL is exactly mkd_sample_dpmpp. */
int mkd_sample_dpmpp_ex(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps, const float* alphas,
                        const float* alphas_prev, int order, int lower_order_final, const mkd_sample_mask* m,
                        const mkd_sample_extras* ex, float cfg_scale, float* x_out, int use_graph, void* stream);
/* ---- UniPC predictor-corrector sampler (Zhao et al. 2023; data prediction, the "bh2" form; BUILD-DEFINED: DESIGN.md §0) -------- */
/* Deterministic, on the same step grid, tables and notation as the DPM-Solver++ entries above.  Grid point k = 0 .. n_steps-1 is the
 * evaluation of executed step k (table entry i = n_steps-1-k, lambda_k from alphas[i]); grid point n_steps is alphas_prev[0].  The
 * corrector walks from one evaluation point to the next, so the table must be contiguous: alphas_prev[i] == alphas[i-1] for i >= 1.
 * With psi_0(h) = 1 - e^-h, psi_j(h) = h^j / j! - psi_{j-1}(h), one update goes from a base s (state x_s, x0-prediction m_s) to lambda_t,
 * h = lambda_t - lambda_s, over q nodes at r_j = (lambda_node_j - lambda_s) / h with d_j = m_node_j - m_s:
 *   U = (sigma_t / sigma_s) x_s + alpha_t (psi_0 m_s + sum_j w_j d_j),   sum_j w_j r_j^i = i! psi_i / h^i  (i = 1 .. q)
 * (exact for an m that is a polynomial of degree q in lambda), except q = 1, where w = psi_0 / (2 r_1): the DPM-Solver++ 2M step as a
 * predictor, and w = psi_0 / 2 for the corrector, whose one node is the new point at r = 1.  Executed step k, with x~_0 = x_T:
 *   1. m_k = (x~_k - sigma_k e_k) / alpha_k, e_k the (guided, possibly rescaled) eps at x~_k
 *   2. k >= 1 and the corrector on: x^c_k = U from base k-1 (x^c_{k-1}, m_{k-1}) to lambda_k over the p_{k-1} - 1 evaluations before
 *      k-1 and m_k at r = 1; otherwise x^c_k = x~_k
 *   3. x~_{k+1} = U from base k (x^c_k, m_k) to lambda_{k+1} over the p_k - 1 previous evaluations
 * p_k = min(order, k + 1), and with lower_order_final != 0 and n_steps < 10 also at most n_steps - k.  The result is x~_{n_steps}: the
 * corrector re-uses the evaluation the next step needs anyway, and there is none after the last one.  As linear forms:
 *   x^c_k = a_c x^c_{k-1} + q_0 m_k + q_1 m_{k-1} + q_2 m_{k-2} + q_3 m_{k-3}        (a_c == 0: no corrector, x^c_k = x~_k)
 *   x~_{k+1} = a_p x^c_k + p_0 m_k + p_1 m_{k-1} + p_2 m_{k-2}
 *
 * mkd_unipc_table: HOST only (no device, no context).  out [n_steps][12] = 1/alpha, sigma, a_c, q_0 .. q_3, a_p, p_0 .. p_2, 0 of table
 * entry i, computed in double and stored as float; step_order [n_steps] (may be NULL) = p_k of entry i.  MKD_ERR_ARG: order outside 1..3,
 * an alpha outside (0, 1), a table that is not contiguous, lambda not increasing along the executed steps. */
int mkd_unipc_table(int n_steps, const float* alphas, const float* alphas_prev, int order, int lower_order_final, int corrector,
                    float* out, int* step_order);
/* One step, one launch: e as in mkd_dpmpp_step; with c = coef12 (HOST, one row of mkd_unipc_table) and x = x~_k:
 * m0_out = (x - c[1] e) c[0];  xc_out = c[2] xc_prev + c[3] m0 + c[4] m1 + c[5] m2 + c[6] m3 (c[2] == 0: xc_out = x);
 * x_next = c[7] xc_out + c[8] m0 + c[9] m1 + c[10] m2.  xc_prev (x^c_{k-1}) and m1 / m2 / m3 (the previous three x0-predictions) are read
 * only where a coefficient of theirs is non-zero and may be NULL otherwise (non-zero with NULL: MKD_ERR_ARG); x_next may alias x and
 * xc_out may alias xc_prev; no other two tensors may overlap.  All fp32 [n]. */
int mkd_unipc_step(const float* x, const float* xc_prev, const float* eps_c, const float* eps_u, float cfg_scale, const float* coef12,
                   const float* m1, const float* m2, const float* m3, float* x_next, float* xc_out, float* m0_out, int64_t n, void* stream);
/* ... with the rescaled eps: k / n_per_sample as in mkd_ddim_step_ex; k == NULL is exactly mkd_unipc_step. */
int mkd_unipc_step_ex(const float* x, const float* xc_prev, const float* eps_c, const float* eps_u, float cfg_scale, const float* coef12,
                      const float* m1, const float* m2, const float* m3, const float* k, int n_per_sample, float* x_next, float* xc_out,
                      float* m0_out, int64_t n, void* stream);
/* The whole loop: mkd_sample_dpmpp's contract (all three loop forms, the same per-step launch count) with the step above as the step's
 * last kernel; the context's history ring has four slots and a buffer for x^c here ([5][B*4*h*w] fp32).  Captured steps are keyed on
 * the solver: DDIM, DPM-Solver++ and UniPC calls may alternate.  m must be NULL: masked sampling with this solver is not defined (the
 * blend would have to act on two carried states): MKD_ERR_UNSUPPORTED, the context stays usable. */
int mkd_sample_unipc(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps, const float* alphas,
                     const float* alphas_prev, int order, int lower_order_final, int corrector, const mkd_sample_mask* m, float cfg_scale,
                     float* x_out, int use_graph, void* stream);
/* mkd_sample_unipc with the trace and the guidance rescale of mkd_sample_extras (trace_x rows are x~_{k+1}, trace_x0 rows m_k);
 * ex == NULL is exactly mkd_sample_unipc. */
int mkd_sample_unipc_ex(mkd_ctx* ctx, const float* x_T, int batch, int n_steps, const int64_t* timesteps, const float* alphas,
                        const float* alphas_prev, int order, int lower_order_final, int corrector, const mkd_sample_mask* m,
                        const mkd_sample_extras* ex, float cfg_scale, float* x_out, int use_graph, void* stream);
/* ---- per-sample requests in one batch (build-defined) ----------------------------------------------------------
 * One request row per sample b: its own schedule (n_steps, 1 <= n_steps <= MKD_MAX_STEPS, and HOST tables laid out as for mkd_sample /
 * mkd_sample_eta: entry n_steps - 1 is executed first) and its own guidance scale.  DDIM (solver 0) reads timesteps, alphas, alphas_prev,
 * sqrt_one_minus_alphas and the optional sigmas; DPM-Solver++ (solver 1) reads timesteps and dpm, the [n_steps][6] table of mkd_dpmpp_table
 * (which carries the sample's order).  The solver is per call. */
#ifndef MKD_MAX_STEPS
#define MKD_MAX_STEPS 1024
#endif
typedef struct mkd_sample_row {
    int32_t n_steps;
    float cfg_scale;
    const int64_t* timesteps;
    const float* alphas; const float* alphas_prev; const float* sqrt_one_minus_alphas;
    const float* sigmas;                 /* NULL: eta = 0 */
    const float* dpm;                    /* solver 1: mkd_dpmpp_table's rows */
} mkd_sample_row;
/* One entry of the per-sample step table: what a sample does in one executed step (64 bytes).  coef = sqrt(1/a_t), sqrt(a_prev),
 * sqrt(1 - a_prev - sigma^2), sqrt(1 - a_t); dpm = a row of mkd_dpmpp_table; temb_row = the row of the call's time-embedding table
 * (one row per distinct timestep of the call, first seen first, steps outer, samples inner) that holds t; active 0: the sample has
 * finished: t / temb_row are those of its entry 0 and its rows are not touched. */
typedef struct mkd_step_row {
    int64_t t;
    float coef[4];
    float sigma;
    float dpm[6];
    int32_t temb_row;
    int32_t active;
    float scale;
} mkd_step_row;
/* HOST only: the step table of a call, out [S_max][batch] with S_max = max_b n_steps (returned in *s_max; pass out NULL to get the
 * sizes alone).  Executed step k = 0 .. S_max - 1; sample b is active while k < n_steps_b and applies its entry n_steps_b - 1 - k
 * (left-aligned: all samples start together, short ones finish first).  distinct [<= MKD_MAX_STEPS] (may be NULL) / *n_distinct: the
 * call's distinct timesteps in first-seen order.  Checks every row first (counts, NULL tables, then with each sample's own tables the
 * sigma range rule of mkd_sample_eta); more than MKD_MAX_STEPS distinct timesteps: MKD_ERR_ARG. */
int mkd_step_table(const mkd_sample_row* rows, int batch, int solver, mkd_step_row* out, int* s_max, int64_t* distinct, int* n_distinct);
/* The whole loop with one request row per sample, all three loop forms (graph replay, its per-stream segments, use_graph == 0, which
 * enqueues the same step kernels uncaptured on `stream` after waiting on the host for the context's previous loop).
 *   - Finished samples: their latent rows (and ring rows) are not written again, whatever the model returns for them; the model is
 *     still evaluated for them at the timestep of their entry 0.
 *   - Guidance: every cfg_scale == 1: the prepared batch is `batch`, nothing is doubled; otherwise it is 2 * batch, unconditional half
 *     first, and every sample uses the guided expression of the uniform kernels with its own scale (a scale of 1 is allowed there).
 *   - eta: noise [S_max][batch * C * h * w] (DDIM; needed when any sigma is non-zero); sample b takes its slice of row k in executed
 *     step k where its sigma is non-zero.  temperature is per call.
 *   - m and ex must be NULL (ex: or ask for neither a trace nor a rescale): masked sampling, the intermediates trace and guidance
 *     rescale are not combined with per-sample rows: MKD_ERR_UNSUPPORTED, the message names the combination.
 * Bit contract: on one context, prepared batch and loop form, row b has the bits of row b of mkd_sample / mkd_sample_eta /
 * mkd_sample_dpmpp run with sample b's request (and rows 0 .. n_steps_b - 1 of the noise).  The per-step launch count is that of the
 * uniform step of the same guidance form under graph replay (mkd_step_launches_ex with MKD_STEP_PER_SAMPLE).  Captured steps are keyed
 * on the per-sample form: uniform and per-sample calls may alternate.  rows and their tables are read before the call returns. */
int mkd_sample_rows(mkd_ctx* ctx, const float* x_T, int batch, const mkd_sample_row* rows, int solver, const float* noise, float temperature,
                    const mkd_sample_mask* m, const mkd_sample_extras* ex, float* x_out, int use_graph, void* stream);
/* The two per-sample updates alone (the eager host-driven loop, tests): rows = DEVICE [batch] entries of one executed step; sample b
 * covers elements [b * n_per_sample, (b + 1) * n_per_sample) of every tensor.  Active samples: the arithmetic of mkd_ddim_step /
 * mkd_dpmpp_step with coef / dpm, scale and sigma of their entry (eps_u NULL: eps_c; noise [batch * n_per_sample] or NULL, read where
 * sigma != 0; pred_x0 may be NULL; x_prev may alias x).  Finished samples: no byte of x_prev / pred_x0 / m0_out is written and nothing
 * of their rows is read.  16-byte accesses when n_per_sample % 4 == 0 and every pointer is 16-byte aligned, scalar otherwise, the same
 * bits.  DPM: m1, m2 (read where the entry's c_1 / c_2 is non-zero) and m0_out are required.  batch <= 65535. */
int mkd_ddim_step_rows(const float* x, const float* eps_c, const float* eps_u, const mkd_step_row* rows, const float* noise, float temperature,
                       float* x_prev, float* pred_x0, int batch, int n_per_sample, void* stream);
int mkd_dpmpp_step_rows(const float* x, const float* eps_c, const float* eps_u, const mkd_step_row* rows, const float* m1, const float* m2,
                        float* x_prev, float* m0_out, int batch, int n_per_sample, void* stream);
/* Latent mask from a label map (reference Fixbackground: labels 0 background, 11 teeth, 12 hair): labels [batch, H, W] uint8
 * device -> out [batch, 1, H/factor, W/factor] fp32 device = the fraction of each factor x factor block whose label l has bit l set
 * in `classes` (labels >= 64 never match): F.interpolate(mode='area') of the binary mask.  threshold > 0: 1 where that fraction
 * >= threshold, else 0.  H, W must be multiples of factor (1..64), else MKD_ERR_ARG. */
int mkd_latent_mask_from_labels(const uint8_t* labels, int batch, int H, int W, uint64_t classes, int factor, float threshold,
                                float* out, void* stream);
/* Pixel-space background paste after the decode (reference Fixbackground.get_target, diffmk/makeup_teacher.py:254-262): image (the decoded
 * sample) and src (the source, both fp32 [batch, channels, H, W] device, nominally [-1, 1]) -> out, per element with ONE correctly rounded
 * fp32 operation per step, in this order (the reference's expression; nothing is contracted to an fma):
 *   u = (s + 1) / 2;  v = (t + 1) / 2;  p = a u;  q = (1 - a) v;  r = p + q;  o = r 2 - 1;  out = min(max(o, -1), 1)
 * with the keep weight a[b,y,x] (1 keeps the source) from exactly ONE of
 *   labels: uint8 [batch, factor H, factor W] device, factor 1..8, `classes` the bit set of mkd_latent_mask_from_labels, feather rho 0..16
 *     image pixels: cnt(y,x) = the label pixels of block (y,x) whose label is in the set; S = sum of cnt over the (2 rho + 1)^2 window,
 *     indices clamped to the image edge; a = float(S) / float((2 rho + 1)^2 factor^2) -- the rule of mkd_region_weights at pixel
 *     resolution.  rho = 0, factor = 1 is the reference's hard mask; rho > 0 is BUILD-DEFINED (the reference has no feather);
 *   mask: fp32 [mask_batch, 1, H, W] device read as is, mask_batch in {1, batch} (1: broadcast); feather must be 0.
 * alpha_out: [batch, 1, H, W] fp32 receives a, or NULL.  out may alias image.  No context; one launch, no scratch buffer, no atomics, no
 * host sync, no allocation: the call only enqueues.  Inputs are finite (NaN behaviour is not specified).  MKD_ERR_ARG before anything
 * is enqueued: both labels and mask or neither, a null image / src / out, factor outside 1..8, feather outside 0..16 or non-zero with a
 * mask, mask_batch not in {1, batch}, channels outside 1..8, batch outside 1..65535, H or W < 1, H * W > 2^24. */
int mkd_paste_background(const float* image, const float* src, const uint8_t* labels, uint64_t classes, int factor, int feather,
                         const float* mask, int mask_batch, float* out, float* alpha_out, int batch, int channels, int H, int W, void* stream);

/* ---- makeup score: region-wise histogram matching (reference diffmk/makeups.py:147-245, diffmk/histogram_matching.py:41-66) ---- */
/* Region mask of a label map (get_msk_lip / get_msk_skin / get_msk_eye, makeups.py:179-230): labels [batch, H, W] uint8 device ->
 * mask_out [batch, H, W] uint8 (1 where label l has bit l set in `classes`; labels >= 64 never match) and count_out [batch] int32, the
 * number of mask pixels.  box_classes != 0 (the eye rule): the mask is kept only inside the bounding box of the labels in box_classes,
 * grown by `margin` pixels on every side and clipped to the image; box_out [batch, 4] int32 (required then) receives that box before
 * growing as (row min, row max, col min, col max), or (INT32_MAX, -1, INT32_MAX, -1) when no pixel carries such a label (the mask is
 * then empty, count 0).  No context, no host sync, no allocation; 2 launches (3 with a box).  batch <= 65535, H * W <= 2^24, else MKD_ERR_ARG. */
int mkd_region_mask_from_labels(const uint8_t* labels, int batch, int H, int W, uint64_t classes, uint64_t box_classes, int margin,
                                uint8_t* mask_out, int32_t* count_out, int32_t* box_out, void* stream);
/* ---- connected components of a label map: every face of a group photo (BUILD-DEFINED; the reference crops ONE detected face) ---- */
/* One component: id = the smallest linear index y W + x of its pixels, area = its pixel count, (r0, r1, c0, c1) = its inclusive
 * bounding box (row min, row max, col min, col max).  24 bytes. */
typedef struct mkd_component { int32_t id, area, r0, r1, c0, c1; } mkd_component;
/* Bytes of device scratch mkd_label_components needs (0 for bad arguments: the limits below).  The scratch must be 256-byte aligned;
 * its contents before the call do not matter (the call initialises what it reads) and it may be reused by the next call on the
 * same stream. */
size_t mkd_label_components_scratch_bytes(int batch, int H, int W);
/* labels [batch, H, W] uint8 device.  A pixel is IN when its label l < 64 has bit l set in `classes` (the rule of
 * mkd_region_mask_from_labels).  Components are the 8-connected sets of in-pixels of one image (4-connectivity is not offered).
 * count [batch] int32 = the number of components of image b with area >= min_area (NOT capped).  table [batch][max_out] =
 * those components ordered by area descending, ties by id ascending, rows 0 .. min(count[b], max_out) - 1; the remaining rows are
 * {-1, 0, INT32_MAX, -1, INT32_MAX, -1} (the empty box of mkd_region_mask_from_labels).  ids_out [batch, H, W] int32 or NULL: the
 * component id at every in-pixel, -1 elsewhere, for ALL components (also those below min_area).  Integer arithmetic only: the outputs
 * are exact and the same bytes on every run.  No context, no host sync, no allocation; 4 launches whatever the data, and no workgroup
 * waits for another.  MKD_ERR_ARG before anything is enqueued unless 1 <= batch <= 65535, H, W >= 1, H * W <= 2^24,
 * 1 <= max_out <= 64, min_area >= 1, labels / table / count / scratch non-null and the scratch 256-byte aligned. */
int mkd_label_components(const uint8_t* labels, int batch, int H, int W, uint64_t classes, int min_area, int max_out,
                         mkd_component* table, int32_t* count, int32_t* ids_out, void* scratch, void* stream);
/* ---- which face owns which pixel: the nearest table component of every pixel (BUILD-DEFINED, as the rest of the group-photo path) ---- */
/* Bytes of device scratch mkd_owner_map needs (0 for bad arguments: the limits below): the column pass's distance (uint16) and rank
 * (uint8) per pixel, each rounded up to 256 bytes.  The scratch must be 256-byte aligned; its contents before the call do not matter
 * and it may be reused by the next call on the same stream. */
size_t mkd_owner_map_scratch_bytes(int batch, int H, int W);
/* Exact Euclidean feature transform.  ids [batch, H, W] int32 device in the form mkd_label_components writes it (the component id at
 * in-pixels, -1 elsewhere), table [batch][max_out] the table of the same call.  The SEEDS of rank r (0 <= r < max_out) of image b are
 * the pixels whose id equals table[b][r].id, for rows with id >= 0; pixels of components that are not in the table (below min_area, or
 * cut off by max_out) are not seeds; of rows that repeat an id the lowest counts.  owner [batch, H, W] uint8 = the rank r that
 * minimises D_r = min over the seeds (v, u) of rank r of (y - v)^2 + (x - u)^2, ties between ranks to the LOWER rank; dist2_out
 * [batch, H, W] int32 or NULL = that minimum.  An image without seeds: owner 255, dist2 INT32_MAX.  The metric is that of the grid
 * the ids live on: face_parser.find_faces squashes a photo to parse_size x parse_size, so in PHOTO pixels the metric is anisotropic
 * (a non-square photo's nearer face is the nearer one of the squashed map).  Integer arithmetic only: the outputs are exact and the
 * same bytes on every run.  No context, no host sync, no allocation, no atomics; 2 launches (per column the nearest seed up or down
 * into the scratch, then per row the smallest (distance, rank) over the columns, scanned outwards from the pixel until the column
 * offset alone exceeds the best distance), and no workgroup waits for another.  MKD_ERR_ARG before anything is enqueued unless
 * 1 <= batch <= 65535, 1 <= H, W <= 2048 (d^2 < 2^23; a row of the intermediate fits in LDS), 1 <= max_out <= 64, ids / table / owner /
 * scratch non-null and the scratch 256-byte aligned. */
int mkd_owner_map(const int32_t* ids, const mkd_component* table, int batch, int H, int W, int max_out, uint8_t* owner,
                  int32_t* dist2_out, void* scratch, void* stream);
/* One face's share of its neighbourhood: items HOST int32 [n][2] = (image, rank), copied into the kernel argument block by value;
 * w_out [n, H, W] fp32: w_out[i][y][x] = float(S) / float((2 rho + 1)^2) with S = the pixels of the (2 rho + 1)^2 window around (y, x),
 * indices clamped to the edge, whose owner [batch, H, W] (mkd_owner_map) equals item i's rank in item i's image -- the window-fraction
 * rule of mkd_region_weights and mkd_paste_background; integers and one division.  feather rho = 0 is the 0 / 1 indicator.  No context;
 * one launch, no scratch, no atomics, no host sync, no allocation.  MKD_ERR_ARG before anything is enqueued unless 1 <= n <=
 * MKD_OWNER_MAX_ITEMS, 0 <= feather <= 16, 1 <= batch <= 65535, 1 <= H, W <= 2048, every image in 0 .. batch - 1 and every rank in
 * 0 .. 63, owner / items / w_out non-null. */
#define MKD_OWNER_MAX_ITEMS 16          /* = MKD_PHOTO_MAX_BATCH: one weight plane per descriptor of a paste */
int mkd_owner_weights(const uint8_t* owner, int batch, int H, int W, const int32_t* items, int n, int feather, float* w_out,
                      void* stream);
/* Bytes of device scratch mkd_hist_match needs for n terms (0 for n <= 0).  The scratch must be 256-byte aligned; its contents
 * before the call do not matter and it may be reused by the next call on the same stream. */
size_t mkd_hist_match_scratch_bytes(int n);
/* Launches one mkd_hist_match call enqueues (memset included) for the outputs asked for: independent of n, at most 5. */
int mkd_hist_match_launches(int want_matched, int want_loss);
/* n independent histogram-matching terms (criterionHis, makeups.py:232-245) in one set of launches.  Term t reads the images
 * dst[index[4t]] and ref[index[4t+1]] (fp32 [3, H, W] each, values clamped to [0, 1]) under the masks mask_dst[index[4t+2]] and
 * mask_ref[index[4t+3]] (uint8 [H, W], non-zero = inside); index == NULL: all four are t.  The caller guarantees that every index
 * lies inside its array.  Per term: v = x * 255 (fp32); per channel 256-bin counts under each mask; pdf = count / total, cdf by
 * sequential fp32 adds; table[i] = the first j in 1..255 with cdf_ref[j-1] <= cdf_dst[i] <= cdf_ref[j], else i (table[0] = 0,
 * table[255] = 255); matched = table[int(v)] under the dst mask, 0 elsewhere; loss = mean over 3 H W of |v mask - matched|.
 * Outputs (each may be NULL, not all of matched / tables / loss): matched [n, 3, H, W] fp32 in 0..255, tables [n, 3, 256] uint8,
 * loss [n] fp32, counts [n, 2] int32 (dst, ref mask pixels).  Tables, matched values and counts equal the reference's; the loss is a
 * fixed-order fp64 sum: the same bits on every run, for every batching of the same terms
 * and for every alignment of the operands (the 16-byte and the scalar load form add a lane's terms in one order).  A term with an empty side (count 0):
 * identity table, matched = 0, loss 0.  Only enqueues.  n <= 65535, H * W <= 2^24, else MKD_ERR_ARG. */
int mkd_hist_match(const float* dst, const float* ref, const uint8_t* mask_dst, const uint8_t* mask_ref, const int32_t* index,
                   int n, int H, int W, float* matched, uint8_t* tables, float* loss, int32_t* counts, void* scratch, void* stream);
/* ---- the histogram-matching teacher: EleGANt's pseudo ground truth at warp weight alpha = 0 (reference teacher.py:96-112), i.e. the
 * region-wise histogram match of the source to the reference composed into one image.  BUILD-DEFINED: region priority, feather and
 * border rule below.  The landmark-warped term (alpha > 0) is mkd_pgt_warp, applied to this image ---- */
/* src [n, 3, H, W] fp32; masks uint8 [4][n][H][W] in the order lip, skin, eye_left, eye_right (non-zero = inside), tables uint8
 * [4][n][3][256] in the same order: the tables of ONE mkd_hist_match call of 4 n terms (term r n + b: dst = source b, ref = reference b
 * under region r's masks); strengths fp32 [n][4] in the same order, or NULL for all 1; out [n, 3, H, W] fp32 in [0, 1].
 *   id(p) = the first of lip (1), eye_left (2), eye_right (3), skin (4) whose mask is non-zero at p, else 0: skin labels overlap the
 *     eye boxes, the priority makes the regions exclusive and the result independent of the evaluation order;
 *   c_r(p) = the number of pixels q of the (2 feather + 1)^2 window around p that lie INSIDE the image and have id(q) = r; K =
 *     (2 feather + 1)^2 always, so outside counts as "no region" (makeup fades towards the image border) and sum_r c_r <= K;
 *   v = clamp(src_c(p), 0, 1) * 255 in fp32 and i = min(int(v), 255), exactly mkd_hist_match's value and bin (NaN -> 0; a zero, also from a source of -0, is +0);
 *   out_c(p) = clamp((v + sum_{r = 1..4} (a_r * (c_r / K)) * (T_{r,c}[i] - i)) / 255, 0, 1)
 * evaluated in double from the fp32 / integer operands, every operation rounded on its own, the terms added in the order r = 1..4,
 * and rounded to fp32 ONCE (tests/teacher_ref.py reproduces the bits).  Consequences: feather 0 and a = 1 give (T_r[i] + (v - i)) / 255
 * inside region r -- mkd_hist_match's matched value / 255 plus the source's sub-bin fraction, which is 0 for a source whose v is a
 * whole number -- and the clamped source elsewhere; an identity table (an empty side of a term) changes nothing; a = 0 gives
 * float(double(v) / 255): a source value float(k / 255) comes back bit for bit, any other within one fp32 ulp.
 * a_r outside [0, 1] is not checked here.  One launch (mkd_pgt_launches), no scratch, no atomics, no host sync, no allocation: the call
 * only enqueues.  No alignment of W or of the pointers beyond 4 bytes for the fp32 arrays is assumed; the 16-byte and the scalar form
 * give the same bits.  MKD_ERR_ARG before anything is enqueued unless 1 <= n <= 65535, H, W >= 1, H * W <= 2^24, 0 <= feather <= 8,
 * src / masks / tables / out non-null, and out does not overlap src. */
int mkd_pgt_compose(const float* src, const uint8_t* masks, const uint8_t* tables, const float* strengths, int n, int H, int W,
                    int feather, float* out, void* stream);
/* Launches one mkd_pgt_compose call enqueues: 1. */
int mkd_pgt_launches(void);
/* ---- the landmark-warped term of the pseudo ground truth: EleGANt's AnnealingComposePGT (reference teacher.py:96-112) warps the
 * reference onto the source through the 68 landmarks by a thin-plate spline and blends it in per region (EYE_ALPHA 0.8, SKIN_ALPHA 0.3,
 * LIP_ALPHA 0.1).  BUILD-DEFINED (EleGANt's own code is not part of the reference): ONE spline per sample through all its control
 * points instead of one per region -- it interpolates every landmark anyway and needs no assignment of landmarks to regions ---- */
/* xh, ref, out fp32 [n, 3, H, W]: xh the alpha = 0 image (mkd_pgt_compose's output), ref the reference; src_masks, ref_masks uint8
 * [4][n][H][W] in the order lip, skin, eye_left, eye_right; ctrl double [n][max_ctrl][2] = the control points (y, x); coef double
 * [n][2][max_ctrl + 3]: row d in {y, x} holds w_d0 .. w_d,K-1 at the front and a_d0, a_d1, a_d2 in the LAST three slots; kcount int32
 * [n]: K_b in 0 .. max_ctrl (a value outside is clamped into that range); alphas fp32 [n, 4] in mask order, in [0, 1] (not checked
 * here, like strengths); map_out double [n][2][H][W] = (q_y, q_x) or NULL.  The spline maps the source pixel p = (y, x) to q in the
 * reference:
 *   s_k  = (y - c_ky)^2 + (x - c_kx)^2;  U(s) = s log(s) for s > 0, else 0 (also for a NaN s);
 *   q_d  = ((sum_{k = 0..K-1} w_dk U(s_k)) + a_d0) + a_d1 y + a_d2 x
 * in double, the sum sequential from +0 in the order k = 0 .. K - 1, the terms added in the order written, every operation rounded on
 * its own (nothing contracts), log = the device's double log.
 *   c_r(p), Kw = (2 feather + 1)^2 and the region ids are mkd_pgt_compose's, from the SOURCE masks;
 *   m'_r(q) = the bilinear sample of "ref_masks plane of region r != 0" (1 / 0), a tap outside the image is 0;
 *   R_c(q)  = the bilinear sample of clamp(ref_c, 0, 1) (NaN -> 0, a zero is +0), tap indices clamped to the image;
 *   both with y0 = floor(q_y), f_y = q_y - y0 (x likewise), top = v00 + f_x (v01 - v00), bot = v10 + f_x (v11 - v10),
 *   v = top + f_y (bot - top), in double, every operation rounded on its own; unless -1 < q_y < H and -1 < q_x < W every m' is 0
 *   (this covers a NaN and a huge q);
 *   Wt       = min(1, sum_{r = 1..4} (alpha_r * (c_r / Kw)) * m'_r(q))   (from +0, in the order r = 1..4; a term with c_r = 0 is +0)
 *   out_c(p) = float(xh_c + Wt * (R_c - xh_c))   (double, ONE rounding to fp32);  Wt = 0: the bits of xh_c.
 * A sample with K_b = 0 has Wt = 0 everywhere: out = xh bit for bit.  Where every c_r(p) is 0 no spline is evaluated (most of the
 * background; a 16 x 16 tile of such pixels copies xh and leaves).  With map_out the spline is evaluated at every pixel of every sample
 * with K_b > 0 and a sample with K_b = 0 writes q = p; the early-out then only skips the sampling.  tests/teacher_warp_ref.py restates
 * all of it; where no log reaches the result (w = 0) the kernel is held to it bit for bit, else within the rounding bound stated there.
 * One launch (mkd_pgt_warp_launches), no scratch, no atomics, no host sync, no allocation: the call only enqueues.  A thread is a pixel
 * for every alignment (there is one load form), so no alignment beyond 4 bytes for the fp32 / int32 arrays and 8 bytes for the double
 * arrays is assumed or can change the bits.  MKD_ERR_ARG before anything is enqueued unless 1 <= n <= 65535, H, W >= 1, H * W <= 2^24,
 * 0 <= feather <= 8, 1 <= max_ctrl <= 128, every pointer but map_out non-null and aligned as above, out does not overlap ref, and out
 * is either xh itself (in place: a pixel reads only its own xh) or does not overlap xh at all. */
int mkd_pgt_warp(const float* xh, const float* ref, const uint8_t* src_masks, const uint8_t* ref_masks, const double* ctrl,
                 const double* coef, const int32_t* kcount, const float* alphas, int n, int H, int W, int max_ctrl, int feather, float* out,
                 double* map_out, void* stream);
/* Launches one mkd_pgt_warp call enqueues: 1. */
int mkd_pgt_warp_launches(void);
/* ---- control points for mkd_pgt_warp without landmarks.  BUILD-DEFINED (the reference takes dlib's 68 landmarks from files): the
 * control points of a face come from the four region masks the teacher already has, and the spline through them is solved on the
 * device.  tests/teacher_points_ref.py restates both calls ---- */
/* masks uint8 [4][n][H][W] in the order lip, skin, eye_left, eye_right (mkd_pgt_compose's; n may count sources and references alike).
 * The regions are made exclusive by mkd_pgt_compose's id(p): lip 1, eye_left 2, eye_right 3, skin 4.  Per image K = 4 (dirs + 1)
 * points, dirs = D in {8, 16}, in the order r = 1..4 and within a region the centroid, then the support points d = 0 .. D - 1:
 *   n_r = the pixels with id r; sy, sx = the int64 sums of their y and x;
 *   centroid = (double(sy) / double(n_r), double(sx) / double(n_r)), one IEEE division each;
 *   support point d = the pixel of the region with the largest int32 projection cq_d x + sq_d y, ties to the smallest linear index
 *     y W + x (one unsigned 64-bit key (proj + 2^31) << 32 | (0xFFFFFFFF - lin), reduced by max);
 *   (cq_d, sq_d), y pointing down, for D = 16: (16384, 0), (15137, 6270), (11585, 11585), (6270, 15137), (0, 16384) for d = 0..4,
 *     d = 5..8 is d' = 8 - d with cq negated, d = 9..15 is d - 8 negated; D = 8 takes every second entry.
 * pts double [n][K][2] = (y, x); use int32 [n][K] = 1 for every point of a region with n_r >= min_area, else 0 and the point is
 * (0, 0); count int32 [n][4] = n_r in the order r = 1..4, or NULL.  Integers and two divisions: the outputs are exact and the same
 * bytes on every run.  Three launches (mkd_region_points_launches: clear, accumulate with 256 threads x 4 consecutive pixels and one
 * global atomic per touched cell of a workgroup, finish), no host sync, no allocation: the call only enqueues.  scratch:
 * mkd_region_points_scratch_bytes(n) bytes on the device.  MKD_ERR_ARG before anything is enqueued unless 1 <= n <= 65535,
 * 1 <= H, W <= 4096, H * W <= 2^24, dirs in {8, 16}, min_area >= 1, masks / pts / use / scratch non-null, pts 8-byte and use / count
 * 4-byte aligned, and the scratch 256-byte aligned. */
int mkd_region_points(const uint8_t* masks, int n, int H, int W, int dirs, int min_area, double* pts, int32_t* use, int32_t* count,
                      void* scratch, void* stream);
/* Bytes of device scratch mkd_region_points needs for n images (76 64-bit cells each, rounded up to 256 bytes; 0 unless 1 <= n <= 65535). */
size_t mkd_region_points_scratch_bytes(int n);
/* Launches one mkd_region_points call enqueues: 3. */
int mkd_region_points_launches(void);
/* The thin-plate splines that carry each sample's source points onto its reference points, in the layout mkd_pgt_warp reads: pts_src,
 * pts_ref double [B][K][2] = (y, x); use_src, use_ref int32 [B][K] or NULL (all 1); ctrl double [B][max_ctrl][2], coef double
 * [B][2][max_ctrl + 3] (the affine part in the LAST three slots of a row), kcount int32 [B]; unused slots are 0.  Per sample:
 *   1. the pairs with both use flags non-zero, in order; a non-finite coordinate in any of them gives K_b = 0;
 *   2. a pair whose source point equals (==, both coordinates) that of an earlier kept pair is dropped; fewer than 3 left: K_b = 0;
 *   3. the (k + 3)^2 system [[U(|c_i - c_j|^2), P], [P^T, 0]] [w; a] = [d; 0], P = [1, y, x], c = the source points, d = the reference
 *      points, s = dy dy + dx dx, U(s) = s log(s) for s > 0, else 0 (log = the device's double log);
 *   4. Gaussian elimination in double with partial pivoting, both right sides along: the pivot of column p is the largest |A[i][p]|,
 *      i >= p, ties to the lowest row (a non-finite entry counts as infinite); a pivot that is 0 or not finite gives K_b = 0;
 *      A[i][j] -= (A[i][p] / pivot) A[p][j]; back substitution x_p = b_p / A[p][p], then b_i -= A[i][p] x_p for i < p, p = k + 2 .. 0;
 *      every operation rounded on its own;
 *   5. the system is built again: a non-finite coefficient, or max |A sol - rhs| over ALL k + 3 rows and both columns (row sums in
 *      the order j = 0 .. k + 2 from +0) above 1e-6, gives K_b = 0;
 *   6. K_b = 0 writes zeros everywhere.
 * One launch (mkd_tps_solve_launches), one workgroup per sample, (max_ctrl + 3) (max_ctrl + 5) doubles of LDS, no atomics and a fixed
 * order of every sum: the same bytes on every run.  No host sync, no allocation.  MKD_ERR_ARG before anything is enqueued unless
 * 1 <= B <= 65535, 1 <= K <= max_ctrl <= 128, pts_src / pts_ref / ctrl / coef / kcount non-null and 8-byte aligned, use_* 4-byte. */
int mkd_tps_solve(const double* pts_src, const double* pts_ref, const int32_t* use_src, const int32_t* use_ref, int B, int K, int max_ctrl,
                  double* ctrl, double* coef, int32_t* kcount, void* stream);
/* Launches one mkd_tps_solve call enqueues: 1. */
int mkd_tps_solve_launches(void);

/* ---- full-resolution photos: crop-resize in, detail-keeping paste out (reference diffdata/preprocessing.py:131-169 crops the face and
 * resizes it to the network size; the paste back is BUILD-DEFINED after the Laplacian detail transfer of PSGAN / EleGANt) ---- */
/* One photo of a batch: interleaved RGB uint8 rows on the device, `pitch_bytes` apart (>= 3 W; NO alignment of pixels or of the pitch
 * is assumed), and the box [x0, x0 + bw) x [y0, y0 + bh) inside it.  labels: uint8 [H][W] contiguous, or NULL.  The HOST array of at
 * most MKD_PHOTO_MAX_BATCH descriptors is copied into the kernel argument block by value; photos of one batch may differ in size.
 * Limits (else MKD_ERR_ARG before anything is enqueued): 1 <= n <= 16, 8 <= S <= 1024, 1 <= H, W <= 16384, pitch_bytes >= 3 W,
 * bw, bh >= 1, the box inside the photo, bw, bh <= 32 S, pixels not NULL. */
#define MKD_PHOTO_MAX_BATCH 16
#define MKD_PHOTO_MAX_FEATHER 64
typedef struct mkd_photo_desc {
    const uint8_t* pixels;
    int32_t pitch_bytes;
    int32_t H, W;
    int32_t x0, y0, bw, bh;
    const uint8_t* labels;
} mkd_photo_desc;
/* Bytes of device scratch mkd_crop_resize needs for these descriptors (0 for bad arguments): per photo the horizontally resized
 * rows the vertical pass reads, uint8 [rows][S][3] with rows <= bh + 2 ceil(max(bh / S, 1)) + 2 (the vertical filter reaches up to
 * its support beyond the box, as the horizontal one does), each slab rounded up to 256 bytes.  The scratch must be 256-byte aligned;
 * its contents before the call do not matter and it may be reused by the next call on the same stream. */
size_t mkd_crop_resize_scratch_bytes(const mkd_photo_desc* descs, int n, int S);
/* Photo box -> S x S with the BYTES of PIL's Image.resize((S, S), Image.BILINEAR, box=(x0, y0, x0 + bw, y0 + bh)) (Pillow's
 * antialiased two-pass integer resampler).  Per axis (input length N, box [in0, in0 + len), output S), in IEEE double, nothing
 * contracted: scale = len / S; fs = max(scale, 1); support = fs; for output index xx: center = in0 + (xx + 0.5) scale;
 * xmin = max(0, (int)(center - support + 0.5)); xmax = min(N, (int)(center + support + 0.5)); for x in xmin .. xmax - 1:
 * w = 1 - |(x - center + 0.5) (1 / fs)| when that absolute value is < 1, else 0; ww = their sum in index order; k = w / ww; integer
 * coefficient (int)(0.5 + k 2^22).  Horizontal pass first (over the photo rows the vertical pass reads), then vertical; every output
 * value is clip((2^21 + sum pixel * coef) >> 22, 0, 255) in 32-bit integers and the intermediate between the passes is uint8.  Both
 * passes always run (at scale 1 with an integer box the coefficients are exactly (1, 0): the same bytes as Pillow's skipped pass).
 * Outputs: img01 fp32 [n, 3, S, S] = float(u8) / 255.0f (one division); u8_out uint8 [n, S, S, 3] or NULL; labels_out uint8 [n, S, S]
 * or NULL (then every descriptor needs labels): labels_out[y][x] = labels[y0 + ((2 y + 1) bh) / (2 S)][x0 + ((2 x + 1) bw) / (2 S)],
 * integer division, no interpolation between classes (BUILD-DEFINED; not Pillow's NEAREST).  img01 and u8_out not both NULL.
 * No context; two launches, no allocation, no host sync, no atomics. */
int mkd_crop_resize(const mkd_photo_desc* descs, int n, int S, float* img01, uint8_t* u8_out, uint8_t* labels_out, void* scratch,
                    void* stream);
/* Debug export of the coefficient table of ONE axis (the device function both passes of mkd_crop_resize run): bounds_out int32
 * [S][2] = (xmin, xmax), coef_out int32 [S][ksize] with ksize = 2 ceil(max(len / S, 1)) + 1, entries past xmax - xmin zero.
 * 1 <= N <= 16384, the box inside, len <= 32 S, 8 <= S <= 1024, else MKD_ERR_ARG. */
int mkd_resize_coeffs(int N, int in0, int len, int S, int32_t* bounds_out, int32_t* coef_out, void* stream);
/* The decoded sample back into the photo, IN PLACE, keeping the photo's fine detail (BUILD-DEFINED): t fp32 [n, 3, S, S] the decoded
 * sample (nominally [-1, 1]), s01 fp32 [n, 3, S, S] the img01 the model saw, the descriptors of mkd_crop_resize (labels unused);
 * pixels is read and WRITTEN inside the box only, every byte outside stays.  feather rho: 0..64 photo pixels.  Every line ONE correctly
 * rounded fp32 operation, nothing contracted.  At model resolution r = (t + 1) 0.5; d = (r - s01) 255.  Per photo pixel and axis, with
 * j = X - x0: num = (2 j + 1) S - bw; den = 2 bw; i0 = floor(num / den); rem = num - i0 den; w = float(rem) / float(den); neighbours
 * clamp(i0, 0, S - 1) and clamp(i0 + 1, 0, S - 1) (half-pixel centres, clamped to the edge).  top = d00 + wx (d01 - d00); bot likewise;
 * u = top + wy (bot - top).  e = distance in pixels to the nearest box side that does not lie on the photo's border (no such side:
 * a = 1); a = float(min(e + 1, rho + 1)) / float(rho + 1); o = float(photo) + a u; out = uint8(clip(rint(o), 0, 255)), ties to even.
 * Bilinear is linear, so this is up(result) + (photo - up(small source)): only the difference is interpolated.  Inputs are finite.
 * No context; one launch, no scratch, no allocation, no host sync, no atomics. */
int mkd_paste_photo(const mkd_photo_desc* descs, int n, int S, const float* t, const float* s01, int feather, void* stream);
/* mkd_paste_photo with one more factor: w fp32 [n, wh, ww] device, a low-resolution weight over the WHOLE photo of descriptor b (not
 * over its box; e.g. mkd_owner_weights on the squashed photo's grid).  Per photo pixel (X, Y) the axis rule above runs on the photo:
 * numx = (2 X + 1) ww - W; denx = 2 W (likewise Y, H, wh; |num| < 2^27 and rem < den <= 32768 hold for W <= 16384, ww <= 2048), which
 * gives the four neighbours w00 .. w11 and the weights ux, uy; then, every line ONE correctly rounded fp32 operation,
 * g = lerp(lerp(w00, w01, ux), lerp(w10, w11, ux), uy) with lerp(p, q, v) = p + v (q - p);  a' = a g;  o = float(photo) + a' u, and the
 * rest as above.  g = 0 leaves the photo's byte as it is (rint(photo + 0) is the byte); w = 1 everywhere gives mkd_paste_photo's
 * bytes.  1 <= wh, ww <= 2048, w non-null, else MKD_ERR_ARG; everything else as mkd_paste_photo.  One launch. */
int mkd_paste_photo_weighted(const mkd_photo_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w,
                             int wh, int ww, void* stream);
/* mkd_paste_photo (w == NULL) / mkd_paste_photo_weighted (w != NULL) with the bilinear interpolation of d replaced by JOINT BILATERAL
 * upsampling under the photo's own edges (Kopf et al. 2007; BUILD-DEFINED): a x5 .. x8 bilinear upsample smears d over a band of photo
 * pixels across a lip line or the jaw, while the photo's edge sits sharp in the middle of that band; here every tap is also weighted by
 * how close the luminance of ITS model pixel is to that of the photo pixel.  radius R: 0, 1 or 2; sigma in 8-bit luminance levels,
 * finite with 0.5 <= sigma <= 1e6; else MKD_ERR_ARG before anything is enqueued.  fp32, every operator below ONE correctly rounded
 * operation, nothing contracted.  Per model pixel: d_c as in mkd_paste_photo; gb_c = clamp(rintf(s01_c * 255.0f), 0, 255) as an integer
 * (the crop's byte when s01 comes from mkd_crop_resize); Yl = float(77 gb_r + 150 gb_g + 29 gb_b) (an integer <= 65280).  Per photo
 * pixel of the box and per axis: the floor quotient q = i0 and the weight w of mkd_paste_photo's axis rule, q NOT clamped (qx, wx, qy,
 * wy); Yh = float(77 R + 150 G + 29 B) of the pixel's own bytes, read before they are written; inv = 1.0f / (256.0f * sigma);
 * invT = 1.0f / float(R + 1).  Taps my = -R .. R + 1 (outer), mx = -R .. R + 1 (inner), both ascending; the model pixel read is
 * (clamp(qy + my, 0, S - 1), clamp(qx + mx, 0, S - 1)) while the spatial weight uses the unclamped offset: per axis
 * dist = float(m) - w for m >= 1 and w + float(-m) for m <= 0; ws = 1.0f - dist * invT (a tent of half-width R + 1 model pixels about
 * the sample point; R = 0 gives the bilinear weights).  Per tap: q = (Yh - Yl) * inv (the difference is exact);
 * wr = 1.0f / (1.0f + q * q) (a Cauchy weight: no exp, never zero); g = (wsy * wsx) * wr; sw = sw + g; sc_c = sc_c + g * d_c, one
 * accumulator per channel and one for the weights, all starting at +0.  u_c = sc_c / sw; sw > 0 always (taps 0 and 1 of an axis never
 * both vanish and wr >= 3.8e-6).  The rest is mkd_paste_photo_weighted unchanged: a, a' = a g_plane when w is given,
 * o = float(photo) + a' u_c, out = uint8(clip(rint(o), 0, 255)).  sigma = 1e6 makes wr 1 to within 2^-24: a tent-weighted average.
 * One thread per photo pixel; every tap reads t and s01 from the L2-resident tensors.  The only photo bytes a thread reads are the
 * ones it writes, so the paste is safe in place.  No context; ONE launch, no scratch, no allocation, no host sync, no atomics. */
int mkd_paste_photo_guided(const mkd_photo_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w,
                           int wh, int ww, int radius, float sigma, void* stream);

/* ---- tilted faces: the photo path along a rotated square (BUILD-DEFINED; the reference aligns nothing, its crops are upright boxes) ---- */
/* One photo of a batch and an ORIENTED square in it.  pixels, pitch_bytes, H, W, labels: as mkd_photo_desc.  Photo coordinates: pixel
 * (X, Y) has its centre at (X + 0.5, Y + 0.5).  (cx, cy) = the square's centre, side = its side in photo pixels, e_u = (c, s) = the unit
 * vector of the face's "right" axis and e_v = (-s, c) that of its "down" axis; c = 1, s = 0 is upright.  The square need NOT lie inside
 * the photo (a rolled face at the border sticks out: the crop replicates edges, the paste writes only what is inside the photo).  The
 * HOST array of at most MKD_PHOTO_MAX_BATCH descriptors is copied into the kernel argument block by value.  Limits (else MKD_ERR_ARG
 * before anything is enqueued): 1 <= n <= 16, 8 <= S <= 1024, 1 <= H, W <= 16384, pitch_bytes >= 3 W, pixels not NULL, cx, cy, side, c,
 * s finite, 0 < side <= 32 S, |c^2 + s^2 - 1| <= 1e-9, -side <= cx <= W + side and -side <= cy <= H + side. */
typedef struct mkd_photo_frame_desc {
    const uint8_t* pixels;
    int32_t pitch_bytes;
    int32_t H, W;
    double cx, cy, side;
    double c, s;
    const uint8_t* labels;
} mkd_photo_frame_desc;
/* Oriented square -> S x S: Pillow's triangle (bilinear, antialiased) filter taken in the face's frame, in ONE pass.  IEEE double
 * throughout, every line below ONE correctly rounded operation per operator, nothing contracted, evaluated left to right with the
 * parentheses shown.  scale = side / S; fs = max(scale, 1); half = side * 0.5; R = fs * (|c| + |s|).  For output (row i, col j):
 * u = ((j + 0.5) * scale) - half; v = ((i + 0.5) * scale) - half; qx = (cx + c * u) - s * v; qy = (cy + s * u) + c * v.  Taps: the integer
 * photo pixels (X, Y) with floor(qx - R) <= X <= floor(qx + R) and floor(qy - R) <= Y <= floor(qy + R) (the tent's support is a
 * rotated square of half-diagonal reach R per axis), Y outer, X inner, both ascending.  Per tap: dx = (X + 0.5) - qx;
 * dy = (Y + 0.5) - qy; du = c * dx + s * dy; dv = c * dy - s * dx; wu = 1 - |du| / fs; wv = 1 - |dv| / fs; a tap with wu <= 0 or
 * wv <= 0 has weight 0 and is skipped (it would add +0.0 to every sum); else w = wu * wv, sw += w and per channel sc += w * byte, the
 * byte read at (clamp(X, 0, W - 1), clamp(Y, 0, H - 1)): edges are replicated.  One accumulator per channel and one for the weights;
 * sw > 0 always (the pixel centre nearest to q lies inside the tent).  u8 = clip(rint(sc / sw), 0, 255), ties to even;
 * img01 = float(u8) / 255.0f.  labels_out[i][j] = labels[clamp(floor(qy), 0, H - 1)][clamp(floor(qx), 0, W - 1)]: classes are never
 * interpolated.  Outputs and their NULL rules as mkd_crop_resize (img01 [n, 3, S, S], u8_out [n, S, S, 3] or NULL, labels_out
 * [n, S, S] or NULL, then every descriptor needs labels; img01 and u8_out not both NULL).  At c = 1, s = 0 and an integer box this is
 * Pillow's filter without its uint8 intermediate and fixed-point coefficients: within 1 of mkd_crop_resize in any byte.  One thread
 * per output pixel, 16 x 16 per workgroup.  No context; ONE launch, no scratch, no allocation, no host sync, no atomics. */
int mkd_crop_frame(const mkd_photo_frame_desc* descs, int n, int S, float* img01, uint8_t* u8_out, uint8_t* labels_out, void* stream);
/* The decoded sample back into the photo along the frame, IN PLACE (t, s01 as mkd_paste_photo).  IEEE double, one correctly rounded
 * operation per operator, nothing contracted.  scale = side / S; half = side * 0.5.  Per photo pixel (X, Y): rx = (X + 0.5) - cx;
 * ry = (Y + 0.5) - cy; u = c * rx + s * ry; v = c * ry - s * rx.  The pixel is INSIDE iff -half <= u < half and -half <= v < half; a
 * pixel outside is neither read for writing nor written.  Per axis (u gives columns, v rows): g = ((u + half) / scale) - 0.5;
 * i0 = floor(g); wx = g - i0; neighbours clamp(i0, 0, S - 1) and clamp(i0 + 1, 0, S - 1).  d = (((double(t) + 1) * 0.5) - double(s01)) * 255
 * at the four neighbours; top = d00 + wx * (d01 - d00); bot likewise; val = top + wy * (bot - top).  e = min(min(u + half, half - u),
 * min(v + half, half - v)); a = min(e + 0.5, rho + 1) / (rho + 1): ALL four sides fade, also one on the photo's border (at roll 0 and
 * an integer box e + 0.5 is mkd_paste_photo's e + 1 for its interior sides).  w != NULL (fp32 [n, wh, ww], the plane of
 * mkd_paste_photo_weighted, 1 <= wh, ww <= 2048): its integers numx = (2 X + 1) ww - W, denx = 2 W, i0 = floor(numx / denx), rem give
 * ux = double(rem) / double(denx) and the neighbours (likewise Y, H, wh); g = lerp(lerp(w00, w01, ux), lerp(w10, w11, ux), uy) with
 * lerp(p, q, k) = p + k * (q - p); a = a * g.  o = double(byte) + a * val; out = uint8(clip(rint(o), 0, 255)), ties to even.  g = 0
 * leaves the byte, w = 1 everywhere gives the bytes of w == NULL.  feather rho: 0..64.  The grid covers the axis-aligned bounding
 * rectangle of the rotated square (centre -+ half * (|c| + |s|) per axis, one pixel of slack per side) clipped to the photo, in
 * 64 x 16 tiles; which pixels are written is decided by the INSIDE test alone.  A square that does not reach its photo writes nothing
 * (no launch when that holds for every descriptor).  No context; ONE launch, no scratch, no allocation, no host sync, no atomics. */
int mkd_paste_frame(const mkd_photo_frame_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w,
                    int wh, int ww, void* stream);
/* mkd_paste_frame with the guided taps of mkd_paste_photo_guided in place of the bilinear interpolation, in IEEE double: per axis
 * g = ((u + half) / scale) - 0.5; q = floor(g) NOT clamped; w = g - q (mkd_paste_frame's own coordinates).  d_c, gb_c, Yl and Yh are
 * formed as in mkd_paste_photo_guided (d_c and Yl in fp32) and widened; inv = 1.0 / (256.0 * double(sigma)); invT = 1.0 / double(R + 1);
 * the taps, their order, dist, ws, q, wr, g, the accumulators and val_c = sc_c / sw are the lines of mkd_paste_photo_guided in double.
 * Then mkd_paste_frame unchanged: a (all four sides fade), a = a * g_plane when w != NULL, o = double(byte) + a * val_c,
 * out = uint8(clip(rint(o), 0, 255)); the INSIDE test alone decides which bytes are read and written, and a square that does not
 * reach its photo writes nothing (no launch when that holds for every descriptor).  radius, sigma and their refusal as in
 * mkd_paste_photo_guided.  No context; ONE launch, no scratch, no allocation, no host sync, no atomics. */
int mkd_paste_frame_guided(const mkd_photo_frame_desc* descs, int n, int S, const float* t, const float* s01, int feather, const float* w,
                           int wh, int ww, int radius, float sigma, void* stream);

/* ---- video clips: the makeup difference filtered over time (BUILD-DEFINED; the reference makes up single images) ---- */
/* A motion-aware recursive filter of d = (t + 1) / 2 - s01 between the decode and the paste of one frame step, for the n faces of that
 * step: t, s01 and t_out are fp32 [n, 3, S, S] with the layout and meaning of mkd_paste_photo (s01 = the crop the model saw, which
 * follows the face, so pixel p is the same place of the face in every frame).  The filtered difference goes back into t_out, which
 * may be t (it must not overlap s01): every paste kernel then sees it, unchanged.  The state is two caller-owned fp32 pools,
 * D_* [pool, 3, S, S] and Y_* [pool, S, S]: face b reads slot slot_in[b] of D_in / Y_in and writes slot slot_out[b] of D_out / Y_out;
 * slot_in and slot_out are HOST arrays [n], copied into the kernel argument block by value.  slot_in[b] = -1: the face has no previous
 * frame.  The caller ping-pongs the pools: the _in pools, D_out and Y_out must not overlap.  fp32, every operator below ONE correctly
 * rounded operation, nothing contracted.  Per model pixel p of face b: gb_c = clamp(rintf(s01_c * 255.0f), 0, 255) as an integer;
 * Y = 77 gb_r + 150 gb_g + 29 gb_b (the luminance of mkd_paste_photo_guided, an integer <= 65280); Y_out[p] = float(Y);
 * d_c = ((t_c + 1.0f) * 0.5f) - s01_c.  slot_in[b] < 0: D_out_c = d_c, t_out_c has the bits of t_c, and no byte of the _in pools is
 * read for this face.  Otherwise, with N = (2 R + 1)^2 and the window (clamp(y + dy, 0, S - 1), clamp(x + dx, 0, S - 1)), dy, dx =
 * -R .. R (edges replicated: always N taps): A = sum |Y(w) - (int)Y_in(w)| in 32-bit integers (exact: any order gives the same bits);
 * inv = 1.0f / ((256.0f * tau) * float(N)); q = float(A) * inv (a uniform change of L grey levels gives q = L / tau);
 * c = 1.0f / (1.0f + q * q) (a Cauchy confidence: no exp, never zero); k = beta * c; D_c = d_c + k * (Din_c - d_c); D_out_c = D_c;
 * t_out_c = ((s01_c + D_c) * 2.0f) - 1.0f.  On a still clip k * 0 = 0 and D = d bit for bit; under stationary noise the temporal
 * variance falls to (1 - beta) / (1 + beta) of the input's.  MKD_ERR_ARG before anything is enqueued: a null pointer, n outside
 * 1 .. MKD_PHOTO_MAX_BATCH, S outside 8..1024, radius outside 0..2, beta not in (0, 0.95], tau not finite in [0.5, 1e6], pool outside
 * 1..65536, a slot_in that is neither -1 nor a slot of the pool, a slot_out outside the pool or repeated, overlapping pools.  One thread per
 * model pixel, 16 x 16 per workgroup, the luminance of the tile plus halo of both frames staged in LDS.  No context; ONE launch, no
 * scratch, no allocation, no host sync, no atomics. */
int mkd_temporal_diff(const float* t, const float* s01, int n, int S, const float* D_in, const float* Y_in, const int32_t* slot_in,
                      float* D_out, float* Y_out, const int32_t* slot_out, int pool, float beta, float tau, int radius, float* t_out,
                      void* stream);

/* Block-matched motion for mkd_temporal_diff (BUILD-DEFINED): the previous state of the n faces of a frame step, fetched through one
 * integer displacement per block of model pixels, so that the filter compares this frame with the previous one where the picture went,
 * not where it was.  s01 [n, 3, S, S], D_in [pool, 3, S, S], Y_in [pool, S, S] and the HOST array slot_in [n] (copied into the kernel
 * argument block by value; -1: no previous frame) are those of mkd_temporal_diff; Y_in holds luminances (0 .. 65280).  D_w / Y_w are a
 * third pair of pools of the same shapes; vec_out is a device int32 [n, nb, nb, 2] = (vy, vx) per block, nb = ceil(S / block), or NULL.
 * Everything is 32-bit integer arithmetic.  Y(p) = 77 gb_r + 150 gb_g + 29 gb_b, gb_c = clamp(rintf(s01_c * 255.0f), 0, 255) (the
 * luminance of mkd_temporal_diff: 256 units are one grey level); Yp(q) = (int)Y_in[slot][q].  A block is block x block model pixels,
 * block 8 or 16; a ragged block at the right or bottom edge covers only its N pixels inside the image.  Candidates v = (vy, vx),
 * vy, vx = -search .. search, search 1..7.  With clamp(p + v) = (clamp(py + vy, 0, S - 1), clamp(px + vx, 0, S - 1)) (edges
 * replicated): SAD(v) = sum over the block's pixels |Y(p) - Yp(clamp(p + v))|; cost(v) = SAD(v) + penalty * N * (|vy| + |vx|), penalty
 * 0..65280 in luminance units per pixel per pixel of displacement (the largest cost is 65280 * 256 * 15 < 2^31).  The block's vector
 * is the lexicographic minimum of (cost, |vy| + |vx|, vy, vx): it does not depend on the order of evaluation, and zero wins every tie
 * it takes part in.  Then for every pixel p of the block, q = clamp(p + v): D_w[slot][c][p] = D_in[slot][c][q] and Y_w[slot][p] =
 * Y_in[slot][q], the bits copied; face b writes the slot it reads, slot_in[b].  A face with slot_in[b] < 0 has zero vectors and no
 * byte of any pool is read or written for it.  The caller passes D_w / Y_w to mkd_temporal_diff as its D_in / Y_in with the same
 * slot_in.  MKD_ERR_ARG before anything is enqueued: a null s01 / pool / slot_in, n outside 1 .. MKD_PHOTO_MAX_BATCH, S outside
 * 8..1024, search outside 1..7, block not 8 or 16, penalty outside 0..65280, pool outside 1..65536, a slot_in that is neither -1 nor a
 * slot of the pool or names a slot twice, D_w / Y_w overlapping D_in / Y_in / s01 or each other.  One workgroup of 256 threads per
 * 16 x 16 pixel tile, both luminances staged in LDS, candidates spread over threads, the minimum reduced as one packed 64-bit key.
 * No context; ONE launch, no scratch, no allocation, no host sync, no atomics. */
int mkd_motion_warp(const float* s01, int n, int S, const float* D_in, const float* Y_in, const int32_t* slot_in, int pool, int search, int block,
                    int penalty, float* D_w, float* Y_w, int32_t* vec_out, void* stream);

/* Every face's roll and its extent in its own frame.  48 bytes: n_a / n_b = the pixels of the component in the class sets a / b (the
 * two eyes), (cq, sq) = the face's "right" axis as integers of length 16384 (16384, 0: upright), umin .. vmax = the component's extent
 * along that axis and the one across it, in units of 1 / (2 S 16384) photo pixel. */
typedef struct mkd_face_frame { int32_t n_a, n_b, cq, sq; int64_t umin, umax, vmin, vmax; } mkd_face_frame;
/* Bytes of device scratch mkd_face_frames needs (six 64-bit moment cells per (image, rank), rounded up to 256 bytes; 0 unless
 * 1 <= batch <= 16 and 1 <= max_out <= 64).  The scratch must be 256-byte aligned; its contents before the call do not matter. */
size_t mkd_face_frames_scratch_bytes(int batch, int max_out);
/* labels uint8 and ids int32 [batch, S, S] device: the square squashed grid of face_parser.find_faces; ids and table [batch][max_out]
 * come from ONE mkd_label_components call.  photo_hw HOST int32 [batch][2] = (H, W) of the photo behind image b, copied into the kernel
 * argument block by value.  frames [batch][max_out] device.  For rank r of image b, over the pixels (x, y) whose id equals
 * table[b][r].id (of rows that repeat an id the lowest counts):
 * MOMENTS (integers): n_a = the pixels whose label l < 64 has bit l set in classes_a, sxa / sya = the sums of their x / y (int64);
 * n_b, sxb, syb likewise for classes_b.
 * DIRECTION (double, one thread): if n_a >= min_eye_area and n_b >= min_eye_area: px = (sxb / n_b - sxa / n_a) * (double(W) / S);
 * py = (syb / n_b - sya / n_a) * (double(H) / S) (the squash is undone: the direction is the photo's); if px < 0 both are negated;
 * len = sqrt(px * px + py * py); cq = (int)rint(px / len * 16384); sq = (int)rint(py / len * 16384).  (cq, sq) = (16384, 0) instead
 * when an eye is missing (below min_eye_area), when len == 0, or when cq < 8192: a roll beyond +-60 degrees is taken as a parser error,
 * not as a pose.
 * EXTENT (int64), over ALL pixels of the component: X2 = (2 x + 1) W; Y2 = (2 y + 1) H (photo coordinates of the pixel centre in
 * units of 1 / (2 S) pixel); pu = cq X2 + sq Y2; pv = -sq X2 + cq Y2 (|.| < 2^43); umin / umax / vmin / vmax = their minima / maxima.
 * A rank whose table id is -1: n_a = n_b = 0, cq = 16384, sq = 0, umin = vmin = INT64_MAX, umax = vmax = INT64_MIN.
 * Sums, minima and maxima are integer atomics, per workgroup in LDS first and then one global 64-bit atomic per non-zero cell; the id
 * -> rank search runs over the table rows in LDS.  Integer outputs: the same bytes on every run (cq, sq come from one thread's
 * doubles).  No context, no host sync, no allocation; 4 launches (clear the moments, moments, direction, extents), 256 threads
 * with 4 consecutive pixels each in the two per-pixel ones, and no workgroup waits for another.  MKD_ERR_ARG before anything is enqueued
 * unless 1 <= batch <= 16, 1 <= S <= 4096, 1 <= max_out <= 64, min_eye_area >= 1, 1 <= H, W <= 16384, labels / ids / table / photo_hw /
 * frames / scratch non-null and the scratch 256-byte aligned. */
int mkd_face_frames(const uint8_t* labels, const int32_t* ids, const mkd_component* table, int batch, int S, int max_out,
                    const int32_t* photo_hw, uint64_t classes_a, uint64_t classes_b, int min_eye_area, mkd_face_frame* frames,
                    void* scratch, void* stream);

/* ---- first-stage decoder ------------------------------------------------ */
/* yaml first_stage_config.params.ddconfig (diffmodels/base_diffusion_makeup.yaml:86-107), decoder half only. */
typedef struct mkd_vae_config {
    int32_t z_channels;      /* 4 */
    int32_t embed_dim;       /* 4 */
    int32_t ch;              /* 128 */
    int32_t n_levels;        /* 4 */
    int32_t ch_mult[8];      /* 1,2,4,4 */
    int32_t num_res_blocks;  /* 2 */
    int32_t out_ch;          /* 3 */
} mkd_vae_config;
/* Adds the "first_stage_model.post_quant_conv.*" / "first_stage_model.decoder.*" entries to the expected state_dict
 * (load them with mkd_load_weight).  Optional: the sampler works without it. */
int mkd_vae_configure(mkd_ctx* ctx, const mkd_vae_config* cfg);
int mkd_vae_finalize(mkd_ctx* ctx);
/* Replaces decode_first_stage (diffmk/diffusion_makeup.py:396,409; diffmk/makeups.py:260-262): z / scale_factor ->
 * post_quant_conv -> Decoder.  z [B,4,h,w] fp32 NCHW -> images [B,3,8h,8w] fp32 NCHW (unclamped, nominally [-1,1]). */
int mkd_decode(mkd_ctx* ctx, const float* z, int batch, int h, int w, float scale_factor, float* images, void* stream);
double mkd_decode_flops(const mkd_ctx* ctx);

/* ---- first-stage encoder ----------------------------------------------------------------------- */
/* Opt-in (a context that only calls mkd_vae_configure expects no encoder key).  Adds "first_stage_model.encoder.*" and
 * "first_stage_model.quant_conv.*" (upstream names) to the expected state_dict; the encoder's input is the yaml's fixed
 * in_channels 3.  Uses ch, ch_mult, n_levels, num_res_blocks, z_channels (4) and embed_dim (4) of `cfg`; out_ch is ignored.
 * Encoder weights are mkd_param_count's which = 4; loading one invalidates the encoder's finalize only. */
int mkd_vae_encoder_configure(mkd_ctx* ctx, const mkd_vae_config* cfg);
int mkd_vae_encoder_finalize(mkd_ctx* ctx);
/* Replaces get_first_stage_encoding(encode_first_stage(x)) (diffmk/makeup_diffuse.py get_z): Encoder -> quant_conv ->
 * DiagonalGaussianDistribution -> sample() (noise != NULL: mean + exp(0.5 clamp(logvar, -30, 20)) * noise) or mode() (noise NULL)
 * -> x scale_factor.  images [B,3,H,W] fp32 NCHW (caller's range, upstream feeds [-1,1]); noise [B,4,H/8,W/8] fp32 device or NULL;
 * z_out [B,4,H/f,W/f] and moments_out [B,8,H/f,W/f] fp32 NCHW (f = 2^(n_levels-1)), each may be NULL but not both.
 * H, W must be multiples of f (else MKD_ERR_ARG); MKD_ERR_STATE when the encoder is not configured.  Its workspace is its own:
 * encoding never moves the decoder's. */
int mkd_encode(mkd_ctx* ctx, const float* images, int batch, int H, int W, float scale_factor, const float* noise, float* z_out,
               float* moments_out, void* stream);
double mkd_encode_flops(const mkd_ctx* ctx);

/* ---- CLIP text encoder -------------------------------------------------- */
/* yaml cond_stage_config FrozenCLIPEmbedder (diffmodels/base_diffusion_makeup.yaml:109-110), i.e. UPSTREAM transformers
 * CLIPTextModel: token + position embeddings, `layers` pre-LN blocks (causal self-attention, quick-GELU MLP), final LN. */
typedef struct mkd_clip_config {
    int32_t vocab_size;      /* 49408 */
    int32_t max_positions;   /* 77 */
    int32_t width;           /* 768 */
    int32_t layers;          /* 12 */
    int32_t heads;           /* 12 */
    int32_t intermediate;    /* 3072 */
    float   ln_eps;          /* 1e-5 */
} mkd_clip_config;
/* Adds the "cond_stage_model.transformer.text_model.*" entries to the expected state_dict.  Optional. */
int mkd_clip_configure(mkd_ctx* ctx, const mkd_clip_config* cfg);
int mkd_clip_finalize(mkd_ctx* ctx);
/* Replaces get_learned_conditioning / FrozenCLIPEmbedder.encode after tokenisation (diffmk/makeup_teacher.py:33-42,
 * diffmk/diffusion_makeup.py:400): tokens [B, n_tokens] int32 (device; padded ids included, CLIP applies only the causal
 * mask) -> last_hidden_state [B, n_tokens, width] fp32 (device). */
int mkd_clip_encode(mkd_ctx* ctx, const int32_t* tokens, int batch, int n_tokens, float* out, void* stream);

/* ---- introspection for bench.py ----------------------------------------------------------- */
/* Executed matmul/conv FLOPs (2 per MAC) of one mkd_eps at the prepared shape. */
double  mkd_eps_flops(const mkd_ctx* ctx);
/* Number of kernel launches of one mkd_eps at the prepared shape. */
int     mkd_eps_launches(const mkd_ctx* ctx);
/* Number of kernel launches of one DDIM step inside mkd_sample at the prepared shape (the time-embedding chain of mkd_eps is
 * computed once per call there, see mkd_sample; + the step setup and the x_{t-1} update). */
int     mkd_step_launches(const mkd_ctx* ctx);                           /* graph replay, no guidance */
int     mkd_step_launches_ex(const mkd_ctx* ctx, int use_graph, int cfg_on); /* as the loop is run: eager adds the timestep fill / table-row select, guidance (cfg_on != 0) the batch doubling, cfg_on == 2 (guidance with rescale) the factor launch */
/* ... cfg_on | MKD_STEP_PER_SAMPLE: a step of mkd_sample_rows (cfg_on & 3 as above; 2 is not built): setup, evaluation, update (+ the batch
 * doubling), the count of the replayed uniform step, whatever use_graph (the per-sample eager loop enqueues the same kernels) */
#define MKD_STEP_PER_SAMPLE 4
/* Kernel classes of the launch plan, and one mkd_eps with a hipEvent pair around every launch group:
 * per-class device milliseconds, executed FLOPs and launch counts (arrays of mkd_kind_count()). Synchronous.
 * csv_path (host string, may be NULL): also write one line per launch group (op,kind,label,ms,gflop). */
int mkd_kind_count(void);
const char* mkd_kind_name(int kind);
int mkd_eps_profile(mkd_ctx* ctx, const float* x, const int64_t* t, float* eps_out, void* stream,
                    double* ms_per_kind, double* flops_per_kind, int* launches_per_kind, const char* csv_path);
/* The same, plus per class: the ALGORITHMIC HBM bytes of the memory-bound launches (GroupNorm / LayerNorm: one read + one write of
 * the tensor; slab-fed GroupNorm: its fp32 slabs in, bf16 out) and the class's launches replayed back to back between ONE event pair
 * (per-launch time without the event overhead of the per-launch pass).  Either array may be NULL. */
int mkd_eps_profile2(mkd_ctx* ctx, const float* x, const int64_t* t, float* eps_out, void* stream,
                     double* ms_per_kind, double* flops_per_kind, int* launches_per_kind, double* bytes_per_kind,
                     double* ms_back_to_back_per_kind, const char* csv_path);
/* Bytes of device memory held by the context (weights + workspace). */
int64_t mkd_device_bytes(const mkd_ctx* ctx);

/* ResBlock tail as ONE implicit GEMM (UPSTREAM ResBlock._forward: out = conv3x3(h) + skip_connection(x), the 1x1 skip of the blocks whose
 * channel count changes; reached from diffmk/makeup_diffuse.py:164-168): y[m, :] = conv3x3(x)[m, :] + x2[m, :] . W_skip^T + bias.
 * w_fold: [N][9 * Cin + K2] bf16, row n = (the packed 3x3 weight row of mkd_pack_conv_weight, tap-major) | W_skip[n, :]; x [batch*H*W, Cin]
 * and x2 [batch*H*W, K2] NHWC at ldx / ldx2; stride 1, pad 1.  Runs on the gather kernel (tile plan of the plain convolution);
 * MKD_ERR_UNSUPPORTED when that shape's plan is an LDS-staged tile. */
int mkd_conv3x3_fold_bf16(const uint16_t* x, int ldx, const uint16_t* w_fold, const float* bias, const uint16_t* x2, int ldx2, int K2,
                          uint16_t* y, int ldy, int batch, int H, int W, int Cin, int N, int splitk, void* stream);

/* ---- single kernels (unit parity tests; bf16 = uint16_t device buffers) -------------------- */
/* C[M,N] = act((A[M,K] . W[N,K]^T + bias[N] + rowbias[m / rows_per_batch][n]) * scale + R[M,N]).
 * conv3x3 != 0: A is NHWC [B,Hin,Win,Cin] (pixel stride lda), K = 9*Cin ordered (ky,kx,ci),
 * output pixel grid Hout x Wout with `stride`, input nearest-upsampled by 2^up first; pad 1.
 * out_f32 selects an fp32 C.  splitk 0 = auto.  act: 0 none, 1 SiLU, 2 GEGLU, 3 quick-GELU, 4 ReLU (applied after the residual). */
int mkd_gemm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias,
                  const float* rowbias, int ldrb, int rows_per_batch,
                  const uint16_t* R, int ldr, float scale, int act,
                  void* C, int ldc, int out_f32, int M, int N, int K,
                  int conv3x3, int batch, int Hin, int Win, int Cin, int Hout, int Wout,
                  int stride, int up, int splitk, void* stream);
/* The VAE encoder's Downsample on the gather kernel: y = conv3x3(F.pad(x, (0,1,0,1)), stride 2, pad 0) + bias.  x NHWC
 * [B,H,W,Cin] (pixel stride ldx), H and W even; w_packed [Cout][3][3][Cin] (mkd_pack_conv_weight); y NHWC [B,H/2,W/2,Cout]
 * (pixel stride ldy).  splitk 0 = auto. */
int mkd_conv3x3_down_bf16(const uint16_t* x, int ldx, const uint16_t* w_packed, const float* bias, uint16_t* y, int ldy,
                          int batch, int H, int W, int Cin, int Cout, int splitk, void* stream);
/* LayerNorm fused into a linear GEMM: C = act(LN(A) . W^T + b) computed as rstd*(A.W'^T - mu*s) + b' on the RAW rows of A.
 * mkd_fold_layernorm builds W' = bf16(W*gamma) (written to rows dst_row0 + n*dst_row_mul of w_out), s = rowsum(W'),
 * b' = bias + W.beta from fp32 W [N,K] (device).  mkd_gemm_ln_bf16 runs the fused GEMM (no split-K).  row_stats == NULL (the
 * form the engine uses): the GEMM takes the row statistics itself from the A fragments it holds (ones . A^T and the diagonal of
 * A . A^T on the matrix cores) - any A, no producer involved.  Otherwise the row sums come from the GEMM that produced A:
 * row_stats [stat_slots][M][2] = partial (sum, sum of squares) per column slot.
 * mkd_gemm_rowstats_bf16 is that producer: C = A.W^T + bias + R (bf16) and the partial row sums of the rounded C. */
int mkd_fold_layernorm(const float* w, const float* gamma, const float* beta, const float* bias, int N, int K,
                       uint16_t* w_out, int dst_row0, int dst_row_mul, float* s_out, float* b_out, void* stream);
int mkd_gemm_ln_bf16(const uint16_t* A, int lda, const uint16_t* Wfold, int ldw, const float* bias_fold, const float* ln_s,
                     const float* row_stats, int stat_slots, float eps, int act, void* C, int ldc, int M, int N, int K,
                     void* stream);
int mkd_gemm_rowstats_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const uint16_t* R, int ldr,
                           uint16_t* C, int ldc, int M, int N, int K, float* stat_out, int stat_capacity_slots, int* slots_out,
                           void* stream);
/* Tuner / tests only: force the GEMM tile configuration (row index of makeupdiffuse_amd/csrc/gemm_tiles.inc; -1 = heuristic). */
int mkd_gemm_force_tile(int cfg);
/* Row `cfg` of the tile-configuration table: block tile (rows x columns), 1 when it is an LDS-staged 3x3 conv tile, its name (static
 * storage).  Returns the number of configurations; fills the outputs (each may be null) only when 0 <= cfg < that.  Needs no device. */
int mkd_gemm_tile_info(int cfg, int* tile_m, int* tile_n, int* lds_staged_conv, const char** name);
/* Tests / experiments: workgroup -> tile order of the GEMM and LDS-staged conv kernels with respect to the 8 XCDs (each has its own
 * L2; workgroups are dealt to them round-robin in launch order).  0 (default): launch order; 1: every XCD gets one contiguous run
 * of the tile sequence with M-tiles fastest (a weight tile lives in one L2); 2: the same with N-tiles fastest.  Results do not
 * depend on it (bit-identical).  Applies to launches issued afterwards. */
int mkd_gemm_set_xcd_mode(int mode);
/* Tests only (race detector): overwrite every buffer one mkd_eps produces (activations, temporaries, workspaces) with NaN
 * patterns, so that a kernel running ahead of its producer cannot see the previous call's values.  Synchronous. */
int mkd_debug_poison(mkd_ctx* ctx);
/* In-eval tuner (tools/tune_ineval.py): per-shape (tile config, split-K) override consulted before the compiled table;
 * cfg < 0 removes one entry, M <= 0 clears all.  Takes effect at the next mkd_prepare (plans re-build). */
int mkd_gemm_set_override(int M, int N, int K, int conv3x3, int stride, int up, int cfg, int splitk);
/* 1 when tile configuration `cfg` can run this shape (the LDS-staged conv tiles have geometry limits). */
int mkd_gemm_cfg_supported(int cfg, int M, int N, int K, int conv3x3, int Hin, int Win, int Cin, int Hout, int Wout,
                           int stride, int up);
/* GroupNorm(32 groups, fp32 statistics) [+SiLU] over NHWC bf16 (pixel stride ld_in). */
int mkd_groupnorm(const uint16_t* x, int ld_in, const float* gamma, const float* beta, float eps,
                  int silu, uint16_t* y, int ld_out, int batch, int hw, int C, int groups, void* stream);
/* GroupNorm split in two so that the statistics pass disappears into the kernel that WRITES the tensor (UPSTREAM GroupNorm32 of
 * ResBlock.in_layers/out_layers and SpatialTransformer.norm, reached from diffmk/makeup_diffuse.py:164-168):
 *   gstat[batch][32][2] = (sum * 2^24, sum of squares * 2^18) as 64-bit integers, zeroed by the caller, accumulated with integer
 *   atomics (order-independent, so results are bit-repeatable) by every producer of the tensor;
 *   mkd_gemm_gnstat_bf16  = mkd_gemm_bf16 whose epilogue also adds the statistics of its bf16 output (columns gn_coff.. of a
 *                           consumer tensor with gn_cg channels per group, gn_hw rows per sample);
 *   mkd_gn_colstats       = stand-alone producer of the same statistics for columns [0, ncols) of x;
 *   mkd_gn_apply_stats    = y = (x - mean) * rstd * gamma + beta [-> SiLU], element-wise, statistics read from gstat. */
int mkd_gemm_gnstat_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias,
                         const float* rowbias, int ldrb, int rows_per_batch,
                         const uint16_t* R, int ldr, float scale, int act, void* C, int ldc, int out_f32, int M, int N, int K,
                         int conv3x3, int batch, int Hin, int Win, int Cin, int Hout, int Wout,
                         int stride, int upsample, int splitk, int64_t* gn_stat, int gn_cg, int gn_coff, int gn_hw, void* stream);
int mkd_gn_colstats(const uint16_t* x, int ld, int batch, int hw, int ncols, int cg, int coff, int64_t* gstat, void* stream);
int mkd_gn_apply_stats(const uint16_t* x, int ld_in, const float* gamma, const float* beta, float eps, int silu, uint16_t* y,
                       int ld_out, int batch, int hw, int C, const int64_t* gstat, void* stream);
/* A split-K GEMM / conv3x3 whose output feeds a GroupNorm(32) [+SiLU]: the GEMM leaves its fp32 partial slabs and ONE kernel does
 * slab reduction + GEMM epilogue (bias, per-sample row bias, scale, residual, bf16 rounding) + GroupNorm -> y; the raw GEMM output
 * is also written to C when write_raw != 0 (C must then be valid).  Same arguments as mkd_gemm_bf16 (act must be 0, bf16 output,
 * rows_per_batch = rows per sample when rowbias is given).  Returns -4 when this shape would not be split over K (splitk = 0 picks
 * the tuned value) or the GroupNorm geometry does not fit the single-pass kernel: call mkd_gemm_bf16 + mkd_groupnorm then. */
int mkd_gemm_groupnorm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias,
                            const float* rowbias, int ldrb, int rows_per_batch,
                            const uint16_t* R, int ldr, float scale, void* C, int ldc, int write_raw, int M, int N, int K,
                            int conv3x3, int batch, int Hin, int Win, int Cin, int Hout, int Wout,
                            int stride, int upsample, int splitk, int rows_per_sample,
                            const float* gamma, const float* beta, float eps, int silu, uint16_t* y, int ld_y, void* stream);
/* ---- fused row-local tail of a SpatialTransformer block (kernels_tfm.hip), stand-alone form ---------------------------------
 * UPSTREAM cldm BasicTransformerBlock after the self-attention product, reached from diffmk/makeup_diffuse.py:164-168:
 *   h1 = attn1.to_out(a1) + h0;  h2 = attn2.to_out(softmax(attn2.to_q(LN2 h1) K^T dh^-0.5) V) + h1;
 *   out = proj_out(ff.net.2(GEGLU(ff.net.0.proj(LN3 h2))) + h2) + x_in
 * as ONE kernel per 64-token row tile (d = 320, 8 heads).  mkd_tfm_tail_create takes the block's fp32 DEVICE weights under their
 * upstream shapes ([d,d], [8d,d], [d,4d], vectors) and builds the packed operand-order copies; mkd_tfm_tail_set_context packs the
 * cross-attention K | V projections of the context (kv: [batch * Tk, 2d] bf16, K in columns [0,d), V in [d,2d); Tk <= 80);
 * mkd_tfm_tail_run: a1, h0, x_in, out are [M, d] bf16 with row strides, M = samples * T, T a multiple of 64.  The engine uses the
 * same kernel inside mkd_eps for its d = 320 blocks (mkd_set_option "tfm_tail"). */
typedef struct mkd_tfm_tail mkd_tfm_tail;
int  mkd_tfm_tail_create(int d, const float* to_out1_w, const float* to_out1_b, const float* norm2_g, const float* norm2_b,
                         const float* to_q2_w, const float* to_out2_w, const float* to_out2_b, const float* norm3_g, const float* norm3_b,
                         const float* ff0_w, const float* ff0_b, const float* ff2_w, const float* ff2_b, const float* proj_out_w,
                         const float* proj_out_b, mkd_tfm_tail** out);
void mkd_tfm_tail_destroy(mkd_tfm_tail* h);
/* Experiment builds (-DMKD_TFM_TRACE) only: device buffer [workgroups][8][32] of int64 time stamps; a no-op in the product build. */
int  mkd_debug_tfm_trace(long long* buf);
int  mkd_debug_attn_trace(long long* buf);      /* -DMKD_ATTN_TRACE builds: [workgroup][wave][8] cycle sums per phase of attention_kernel */
int  mkd_tfm_tail_set_context(mkd_tfm_tail* h, const uint16_t* kv, int ldkv, int batch, int Tk, void* stream);
int  mkd_tfm_tail_run(mkd_tfm_tail* h, const uint16_t* a1, int lda, const uint16_t* h0, int ldh, const uint16_t* xin, int ldx,
                      uint16_t* out, int ldo, int M, int T, void* stream);
/* The head of the same block as ONE kernel behind a GroupNorm statistics launch: GroupNorm(32, eps) apply -> proj_in -> LayerNorm 1
 * folded into to_q | to_k | to_v: x [B * T, d] (row stride ldx, T a multiple of 64) -> h0 [B * T, d] and qkv [B * T, 3d] (dense).
 * fp32 DEVICE weights under their upstream shapes (SpatialTransformer.norm, .proj_in; transformer_blocks.0.norm1, attn1.to_q/k/v). */
typedef struct mkd_tfm_head mkd_tfm_head;
int  mkd_tfm_head_create(int d, const float* gn_g, const float* gn_b, const float* proj_in_w, const float* proj_in_b, const float* norm1_g,
                         const float* norm1_b, const float* to_q_w, const float* to_k_w, const float* to_v_w, mkd_tfm_head** out);
void mkd_tfm_head_destroy(mkd_tfm_head* h);
int  mkd_tfm_head_run(mkd_tfm_head* h, const uint16_t* x, int ldx, float gn_eps, uint16_t* h0, uint16_t* qkv, int batch, int T, void* stream);
/* LayerNorm over the last dim of [rows, d] bf16. */
int mkd_layernorm(const uint16_t* x, const float* gamma, const float* beta, float eps,
                  uint16_t* y, int rows, int d, void* stream);
/* ... with a row stride on x (the engine normalises the h2 columns of its [gg | h2] buffer); y is dense. */
int mkd_layernorm_ld(const uint16_t* x, int ldx, const float* gamma, const float* beta, float eps,
                     uint16_t* y, int rows, int d, void* stream);
/* softmax(q k^T * scale) v per (batch, head); q rows b*Tq+i, k/v rows b*Tk+j, head h at column h*dh. */
int mkd_attention(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv,
                  uint16_t* o, int ldo, int batch, int Tq, int Tk, int heads, int dh, float scale,
                  void* stream);
/* same with the causal mask of the CLIP text encoder: query i attends keys 0..i (Tq == Tk). */
int mkd_attention_causal(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv,
                         uint16_t* o, int ldo, int batch, int Tq, int Tk, int heads, int dh, float scale,
                         void* stream);
/* y[m, j] = x[m, j] * gelu_erf(x[m, inner + j]). */
int mkd_geglu(const uint16_t* x, uint16_t* y, int rows, int inner, void* stream);
/* ---- the side networks' small kernels, one launch each (unit tests; the plans call the same launchers) ---- */
/* y[r, :] = softmax(x[r, :]): x fp32 [rows, cols] (the first-stage mid attention keeps its scores in fp32), y bf16 [rows, cols]. */
int mkd_softmax_rows(const float* x, uint16_t* y, int rows, int cols, void* stream);
/* Fused tail of the first-stage encoder: conv_out (3x3 pad 1, Cin -> 2Z; x bf16 NHWC [batch,H,W,Cin], w packed bf16 [2Z][3][3][Cin], bias
 * fp32 [2Z]) -> quant_conv (wq bf16 [2Z][2Z], bq fp32 [2Z]) -> moments fp32 NCHW [batch,2Z,H,W] = (mean | logvar) and
 * z fp32 NCHW [batch,Z,H,W] = (mean + exp(0.5 clamp(logvar, -30, 20)) * noise) * scale; noise NULL: z = mean * scale.  Either output may
 * be NULL, not both.  z_channels must be 4 and Cin a multiple of 8, else MKD_ERR_ARG. */
int mkd_vae_enc_tail(const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* wq, const float* bq, const float* noise,
                     float scale, float* z_out, float* moments_out, int batch, int H, int W, int Cin, int z_channels, void* stream);
/* post_quant_conv: out[b, o, p] = bias[o] + sum_i w[o, i] * (z[b, i, p] * inv_scale); z, out fp32 [batch, C, hw], w bf16 [C][C]. */
int mkd_post_quant(const float* z, const uint16_t* w, const float* bias, float inv_scale, float* out, int batch, int C, int hw, void* stream);
/* out[b] = [cos(t_b f_k) | sin(t_b f_k)], f_k = exp(-ln(1e4) k / (dim/2)): t int64 [batch] (device), out bf16 [batch, dim]; dim even. */
int mkd_timestep_embedding(const int64_t* t, uint16_t* out, int batch, int dim, void* stream);
/* out[b, t, :] = tok_emb[tokens[b, t]] + pos_emb[t]: tokens int32 [batch, T], tok_emb bf16 [vocab, width], pos_emb bf16 [>= T, width],
 * out bf16 [batch, T, width]; width a multiple of 8.  Ids outside [0, vocab) are clamped (mkd_clip_encode rejects them before). */
int mkd_clip_embed(const int32_t* tokens, const uint16_t* tok_emb, const uint16_t* pos_emb, uint16_t* out, int batch, int T, int width,
                   int vocab, void* stream);
/* y[s] = (1 - alpha[s]) a[s] + alpha[s] b[s] per sample s: a, b, y bf16 [batch, per_sample], alpha fp32 [batch]; per_sample % 8 == 0. */
int mkd_blend_bf16(const uint16_t* a, const uint16_t* b, const float* alpha, uint16_t* y, int64_t per_sample, int batch, void* stream);
/* direct 3x3 conv, pad 1, fp32 accumulate.  in_nchw_f32: x is fp32 NCHW else bf16 NHWC;
 * out_nchw_f32 likewise; act 1 = SiLU; add (bf16 NHWC, may be NULL) is added after act. */
int mkd_conv3x3_direct(const void* x, int in_nchw_f32, const uint16_t* w, const float* bias,
                       void* y, int out_nchw_f32, int act, const uint16_t* add,
                       int batch, int Hin, int Win, int Cin, int Cout, int stride, void* stream);
/* fp32 [Cout,Cin,kh,kw] -> bf16 [Cout][kh][kw][Cin]. */
int mkd_pack_conv_weight(const float* w, uint16_t* out, int Cout, int Cin, int kh, int kw, void* stream);

/* ---- face parsing: label maps from images (csrc/parser.hip, csrc/kernels_parser.hip) --------------------------------------------
 * UPSTREAM zllrunning/face-parsing.PyTorch model.py / resnet.py (BiSeNet, ResNet-18 context path) as vendored by PSGAN / EleGANt
 * faceutils/mask; the reference runs it in diffdata/preprocessing.py:38,151-157.  A stand-alone handle like mkd_tfm_tail, not a plan
 * of mkd_ctx.  Widths, blocks per layer, the context-path / fusion widths and the class count are configuration: every width a
 * multiple of 8 (widths[0] <= 128: the stem's weights live in LDS), n_classes 2..32, ffm_channels a multiple of 8 (its inner width
 * is ffm_channels / 4).  State-dict names are upstream's (cp.resnet.*, cp.arm16|arm32.*, cp.conv_head16|conv_head32|conv_avg.*,
 * ffm.*, conv_out.*); the training-only heads conv_out16.* / conv_out32.* and *.num_batches_tracked are accepted and ignored.
 *
 * mkd_parser_create, _param_*: HOST only, no device call.  mkd_parser_load_weight takes fp32 HOST data; an unknown or wrongly shaped
 * tensor is MKD_ERR_ARG; loading after a finalize asks for another finalize.  mkd_parser_finalize checks completeness
 * (MKD_ERR_MISSING names the first missing tensor), folds every BatchNorm in fp32 (W' = W g / sqrt(var + eps), b' = beta - mean g /
 * sqrt(var + eps)), rounds the GEMM weights to bf16 and uploads them; synchronous.
 *
 * mkd_parser_logits: images01 fp32 NCHW [batch,3,H,W] in [0,1] (device) -> logits_nchw fp32 [batch,n_classes,H/8,W/8] (device).
 * mkd_parser_parse: the same, then the head below at parse size (H, W) -> labels uint8 [batch,out_h,out_w] (device); lut is a HOST
 * table of n_classes bytes or NULL; logits_nchw may be NULL.  batch 1..64, H and W multiples of 32 in 64..1024, out_h / out_w >= 1,
 * else MKD_ERR_ARG before anything is enqueued; MKD_ERR_STATE before finalize.  Calls only enqueue, except that a call whose
 * (batch, H, W) needs more than the handle's workspace holds re-allocates it first (synchronising), as mkd_prepare does.
 * mkd_parser_flops: 2 x the multiply-accumulates of one image; mkd_parser_launches: kernels the last call enqueued. */
typedef struct mkd_parser mkd_parser;
typedef struct mkd_parser_config {
    int32_t n_classes;      /* 19 */
    int32_t widths[4];      /* 64,128,256,512 */
    int32_t blocks[4];      /* 2,2,2,2 */
    int32_t cp_channels;    /* 128 */
    int32_t ffm_channels;   /* 256 (FFM inner = /4) */
    float   bn_eps;         /* 1e-5 */
    float   mean[3], std[3];
} mkd_parser_config;
int  mkd_parser_create(const mkd_parser_config* cfg, mkd_parser** out);
void mkd_parser_destroy(mkd_parser* p);
int  mkd_parser_param_total(const mkd_parser* p);                          /* sorted by name */
const char* mkd_parser_param_name(const mkd_parser* p, int i);
int  mkd_parser_param_shape(const mkd_parser* p, int i, int64_t* shape4);   /* returns ndim <= 4 */
int64_t mkd_parser_param_count(const mkd_parser* p);
int  mkd_parser_load_weight(mkd_parser* p, const char* name, const float* data, int ndim, const int64_t* shape);
int  mkd_parser_finalize(mkd_parser* p);
int  mkd_parser_logits(mkd_parser* p, const float* images01, int batch, int H, int W, float* logits_nchw, void* stream);
int  mkd_parser_parse(mkd_parser* p, const float* images01, int batch, int H, int W, int out_h, int out_w, const uint8_t* lut, uint8_t* labels,
                      float* logits_nchw, void* stream);
double mkd_parser_flops(const mkd_parser* p, int H, int W);
int  mkd_parser_launches(const mkd_parser* p);
/* The head alone, context-free, one launch, no H x W x classes tensor.  logits[b, c, y, x] is read at b s_batch + c s_class + y s_row +
 * x s_col (element strides: NCHW and NHWC run the same code).  For output pixel (oy, ox) of the out_h x out_w map: the parse-resolution
 * pixel is py = (oy P_h) / out_h, px = (ox P_w) / out_w (integer division: the reference's nearest resize, preprocessing.py:154-157);
 * ry = (h8 > 1 && P_h > 1) ? float(h8 - 1) / float(P_h - 1) : 0, fy = float(py) ry, y0 = min((int)fy, h8 - 1), y1 = min(y0 + 1, h8 - 1),
 * wy = fy - float(y0), likewise x (bilinear, align_corners = True); per class top = v00 + wx (v01 - v00), bot = v10 + wx (v11 - v10),
 * val = top + wy (bot - top), every operation one correctly rounded fp32 operation, nothing contracted.  The label is the FIRST class
 * with the largest val, passed through lut (HOST, n_classes bytes) when given.  This arithmetic is build-defined: torch weighs the four
 * corners in another order, so labels can differ from torch's at near-ties only.  Inputs are finite.  n_classes 2..32, batch 1..65535,
 * sizes 1..16384, else MKD_ERR_ARG before anything is enqueued. */
int  mkd_parse_labels(const float* logits, int64_t s_class, int64_t s_row, int64_t s_col, int64_t s_batch, int batch, int n_classes,
                      int h8, int w8, int P_h, int P_w, int out_h, int out_w, const uint8_t* lut, uint8_t* labels, void* stream);
/* Single kernels of the network (unit tests), device pointers:
 * mkd_parser_stem: images01 fp32 NCHW [batch,3,H,W] -> y bf16 NHWC [batch,H/4,W/4,C0] = maxpool3x3_s2_p1(relu(conv7x7_s2_p3((x - mean) /
 *   std) + bias)); the zero padding applies to the normalised image.  w_packed bf16 [(ky*7+kx)*3+c][C0] and bias [C0] carry the folded
 *   BatchNorm; mean3 / std3 are HOST; half_res is scratch for bf16 [batch,H/2,W/2,C0].  Two launches.  C0 % 8 == 0, <= 128; H, W % 32 == 0.
 * mkd_channel_gate: x bf16 NHWC [batch,pixels,C] (pixel stride ldx) -> out fp32 [batch, n2 or n1]: the per-channel mean over the pixels
 *   in fp32 in a FIXED order (same bits every run and for every batch size), then act1(W1 mean + b1) and, when w2 is given,
 *   act2(W2 . + b2); w1 [n1][C], w2 [n2][n1] fp32, biases may be NULL; act 0 none, 1 ReLU, 2 1 / (1 + expf(-x)).  One workgroup per sample.
 * mkd_gate_apply_bf16: y[b,Y,X,c] = bf16(float(x[b,Y>>u,X>>u,c]) a[b,c] + add), x [batch,h,w,C], y [batch,h<<u,w<<u,C], u 0 or 1;
 *   mode 0: add = the fp32 vector add[b,c]; 1: add = the bf16 tensor add[b,Y>>u,X>>u,c] (pixel stride ldadd); 2: add = x itself.  One fp32
 *   product, one fp32 sum, one bf16 rounding. */
int  mkd_parser_stem(const float* images01, const uint16_t* w_packed, const float* bias, const float* mean3, const float* std3, uint16_t* half_res,
                     uint16_t* y, int batch, int H, int W, int C0, void* stream);
int  mkd_channel_gate(const uint16_t* x, int ldx, int batch, int pixels, int C, const float* w1, const float* b1, int n1, int act1, const float* w2,
                      const float* b2, int n2, int act2, float* out, void* stream);
int  mkd_gate_apply_bf16(const uint16_t* x, int ldx, const float* a, int mode, const void* add, int ldadd, uint16_t* y, int ldy, int batch, int h, int w,
                         int C, int u, void* stream);

/* ---- counter-based noise (BUILD-DEFINED: the reference draws torch.randn on a global generator, diffmk/cddim.py:74-78) -------------
 * Element e of row r of sample b is a pure function of (seed_b, sub_b, stream_id, r, e): no state is carried from call to call and
 * nothing depends on the batch, so a sample gets the same noise alone, in any batch and at any position in it.
 *   per sample b   seed_b: 64 bits (carried as int64, the bits of a uint64); sub_b: a 32-bit sub-stream, 0 where subs == NULL (the photo
 *                  path passes the face's rank)
 *   per call       stream_id: what the draw is for.  0 the start latent, 1 a step's eta noise, 2 the masked blend's q_sample noise,
 *                  3 the first-stage posterior; 4..15 reserved; 16 and above free for callers
 *   per row        r = row0 + i for row i of out: the executed step k for streams 1 and 2, 0 otherwise
 * Block j covers elements 4j .. 4j + 3 of a sample's row:
 *   (r0, r1, r2, r3) = Philox4x32-10(counter = (j, r, stream_id, sub_b), key = (seed_b & 0xffffffff, seed_b >> 32))
 * with the multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57 and the Weyl constants 0x9E3779B9, 0xBB67AE85 (Salmon et al. 2011; Random123's
 * philox4x32_R at ten rounds).  A round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
 *   (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))
 * and the key then advances by the Weyl constants.  u(w) = ((w >> 8) + 0.5) 2^-24 lies strictly inside (0, 1) and is exact in double (an odd numerator of up to
 * 25 bits over 2^25: fp32 holds it only below a half).  With
 * rho = sqrt(-2 ln u(r0)): element 4j = rho cospi(2 u(r1)), element 4j + 1 = rho sinpi(2 u(r1)); elements 4j + 2 and 4j + 3 are the same
 * from (r2, r3).  Evaluated in double (log, sqrt, sincospi) and rounded to fp32 once, so |z| <= sqrt(50 ln 2) = 5.887.
 * kind 0: the normals, fp32; kind 1: the raw words r0 .. r3 as uint32 (tests).  out is [rows][batch][n_per_sample], the layout
 * mkd_sample_eta and mkd_sample_mask take for their noise; elements at or beyond n_per_sample are not written.  16-byte stores where out
 * is 16-byte aligned and n_per_sample % 4 == 0, scalar stores otherwise, the same bits.  One launch, no context, no scratch, no host
 * synchronisation, no atomics; capturable.  MKD_ERR_ARG before anything is enqueued: null seeds / out, batch, rows or n_per_sample
 * < 1, kind outside 0..1, ceil(n_per_sample / 4) or row0 + rows - 1 beyond 32 bits (each is one counter word). */
int  mkd_noise_fill(const int64_t* seeds, const int32_t* subs, int batch, uint32_t stream_id, uint32_t row0, int rows, int64_t n_per_sample,
                    int kind, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MKD_H */
