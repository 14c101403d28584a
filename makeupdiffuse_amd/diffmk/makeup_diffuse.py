"""``diffmk.makeup_diffuse`` — inference-side drop-in for the reference model classes on the hot path.

Mirrors, for the DDIM sampling path only:
  * ``apply_model``                 reference diffmk/makeup_diffuse.py:152-170
  * ``get_input`` cond assembly     reference diffmk/makeup_diffuse.py:42-57, diffmk/makeup_controlnet.py:137-167
  * ``sample_log`` / ``log_results``reference diffmk/diffusion_makeup.py:360-411 (UPSTREAM ControlLDM.sample_log)
Training losses, the GAN teachers, PL hooks and the VAE/CLIP stages are out of scope for this path (the histogram-matching
teacher is in: makeupdiffuse_amd/teacher.py, TestDiffuseModel(teacher='hist'));
calling them raises NotImplementedError rather than returning something different from the reference.
The arithmetic runs in libmkd (HIP); there is no CPU implementation behind these classes."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import torch

from ..ddim import DDIMSampler
from ..dpm_solver import DPMSolverSampler
from ..unipc import UniPCSampler
from ..video import TemporalFilter
from ..engine import ClipConfig, MkdEngine, NetConfig, VaeConfig
from ..lib import MkdError
from ..sampling import SOLVERS
from ..schedule import DDIMSchedule


class _Held:
    """Cache key over tensors that HOLDS them: identity + in-place version.  An address-based key would match a new tensor
    that the caching allocator placed where a freed one used to be (the next batch of a test loop: same shapes, same
    allocation order) and silently reuse the previous batch's conditioning."""

    def __init__(self, tensors, extra=()):
        self.tensors = tuple(tensors)
        self.versions = tuple(None if t is None else t._version for t in self.tensors)
        self.extra = tuple(extra)

    def matches(self, tensors, extra=()) -> bool:
        tensors = tuple(tensors)
        return (len(tensors) == len(self.tensors) and tuple(extra) == self.extra
                and all(a is b and (a is None or a._version == v) for a, b, v in zip(tensors, self.tensors, self.versions)))


class BaseMakeUpDiffuse:
    """ControlLDM-shaped inference model: ControlNet(hint = src ‖ ref) -> 13 residuals -> ControlledUnet."""

    def __init__(self, control_stage_config: dict, unet_config: dict, first_stage_config: Optional[dict] = None,
                 cond_stage_config: Optional[dict] = None, linear_start: float = 0.00085, linear_end: float = 0.0120,
                 timesteps: int = 1000, beta_schedule: str = 'linear', scale_factor: float = 0.18215,
                 only_mid_control: bool = False, parameterization: str = 'eps', channels: int = 4, image_size: int = 64,
                 conditioning_key: str = 'crossattn', first_stage_key: str = 'jpg', cond_stage_key: str = 'txt',
                 control_key: str = 'ref_img', src_key: str = 'src_img', src_img_key: str = 'src_img',
                 ref_img_key: str = 'ref_img', use_ema: bool = False, first_stage_encoder: bool = False, **unused_training_params):
        if parameterization != 'eps':
            raise NotImplementedError("parameterization must be 'eps' (base_diffusion_makeup.yaml:50)")
        self.net_config = NetConfig.from_yaml_params(dict(control_stage_config.get('params', control_stage_config)),
                                                     dict(unet_config.get('params', unet_config)))
        self.first_stage_config, self.cond_stage_config = first_stage_config, cond_stage_config
        self.vae_config = None
        if first_stage_config is not None:
            self.vae_config = VaeConfig.from_yaml_params(dict(first_stage_config.get('params', first_stage_config)))
        # opt-in first-stage ENCODER (encode_first_stage / get_z): configured on the device next to the decoder
        self.first_stage_encoder = bool(first_stage_encoder)
        if self.first_stage_encoder and self.vae_config is None:
            raise ValueError('first_stage_encoder=True needs a first_stage_config (its ddconfig describes the encoder)')
        self.clip_config = None
        if cond_stage_config is not None:
            self.clip_config = ClipConfig.from_yaml_params(cond_stage_config.get('params'))
        self.extra_params = dict(unused_training_params)      # w_idt_src, lambda_lip, teacher_type, ... (training only)
        self.parameterization = parameterization
        self.only_mid_control = bool(only_mid_control)
        self.control_scales: List[float] = [1.0] * self.net_config.n_control
        self.scale_factor, self.channels, self.image_size = scale_factor, channels, image_size
        self.conditioning_key = conditioning_key
        self.first_stage_key, self.cond_stage_key, self.control_key = first_stage_key, cond_stage_key, control_key
        self.src_img_key = src_img_key if src_img_key else src_key
        self.ref_img_key = ref_img_key if ref_img_key else control_key
        self.linear_start, self.linear_end = linear_start, linear_end
        self.device = torch.device('cpu')
        self.register_schedule(beta_schedule=beta_schedule, timesteps=timesteps, linear_start=linear_start, linear_end=linear_end)
        self.engine: Optional[MkdEngine] = None
        self._pending_sd: Optional[Dict[str, torch.Tensor]] = None
        self._bound = None
        self._cfg_cache = None
        self._cat_cache = None
        self.cond_stage_model = None          # callable(list[str]) -> [B,77,768]; built on .cuda() when cond_stage_config is set
        self.training = False

    _SCHEDULE_TABLES = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod',
                        'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod')

    def register_schedule(self, given_betas=None, beta_schedule: str = 'linear', timesteps: int = 1000, linear_start: float = 1e-4,
                          linear_end: float = 2e-2, cosine_s: float = 8e-3) -> None:
        """UPSTREAM DDPM.register_schedule as the reference calls it (diffmk/makeups.py:40-42, ``update_schedule``): (re)builds
        the beta / alphas_cumprod tables for ``timesteps`` steps.  Samplers built afterwards see the new ``num_timesteps``."""
        if given_betas is not None:
            raise NotImplementedError('given_betas (the reference passes None, diffmk/makeups.py:41)')
        sch = DDIMSchedule(int(timesteps), linear_start, linear_end, beta_schedule)
        self.schedule = sch
        self.num_timesteps = sch.num_timesteps
        self.linear_start, self.linear_end = linear_start, linear_end
        for n in self._SCHEDULE_TABLES:
            setattr(self, n, getattr(sch, n).to(self.device))

    # ---- nn.Module-ish surface used by runs/test.py --------------------------------------------------------
    def cpu(self):
        return self

    def eval(self):
        self.training = False
        return self

    def cuda(self, device=None):
        return self.to(torch.device('cuda', torch.cuda.current_device() if device is None else device))

    def to(self, device):
        device = torch.device(device)
        if device.type == 'cuda':
            if self.engine is None:
                self.engine = MkdEngine(self.net_config, device)
                if self.vae_config is not None:
                    self.engine.configure_vae(self.vae_config)
                if self.first_stage_encoder:
                    self.engine.configure_vae_encoder(self.vae_config)
                if self.clip_config is not None:
                    from ..clip import FrozenCLIPEmbedder, load_tokenizer
                    self.engine.configure_clip(self.clip_config)
                    params = dict((self.cond_stage_config or {}).get('params') or {})
                    tok_dir = params.get('tokenizer_path') or params.get('version')
                    tok = load_tokenizer(tok_dir) if tok_dir and os.path.isdir(str(tok_dir)) else None
                    self.cond_stage_model = FrozenCLIPEmbedder(self.engine, tok, max_length=self.clip_config.max_positions)
                if self._pending_sd is not None:
                    self.engine.load_state_dict(self._pending_sd, strict=True)
                    self._pending_sd = None
            for n in ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod',
                      'sqrt_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod'):
                setattr(self, n, getattr(self, n).to(device))
            self.device = device
        return self

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """Accepts an upstream-named checkpoint dict (runs/test.py:59-60).  Keys outside the two nets
        (first_stage_model.*, cond_stage_model.*, teacher_model*) are reported back as unexpected."""
        sd = state_dict.get('state_dict', state_dict)
        if self.engine is not None:
            unused = self.engine.load_state_dict(sd, strict=strict)
        else:
            self._pending_sd = {k: v for k, v in sd.items()
                                if k.startswith(MkdEngine.UNET_PREFIX) or k.startswith(MkdEngine.CONTROL_PREFIX)
                                or k.startswith('first_stage_model.post_quant_conv.') or k.startswith('first_stage_model.decoder.')
                                or (self.first_stage_encoder and k.startswith(MkdEngine.VAE_ENCODER_PREFIXES))
                                or (k.startswith(MkdEngine.CLIP_PREFIX) and not k.endswith('position_ids'))}
            unused = [k for k in sd if k not in self._pending_sd]
        return [], unused

    def _require_engine(self) -> MkdEngine:
        if self.engine is None:
            raise MkdError('model is not on a HIP device: call .cuda() first (the hot path has no CPU implementation)')
        return self.engine

    # ---- conditioning -------------------------------------------------------------------------------------
    def get_origin_img_input(self, batch: dict, k: str, bs: Optional[int] = None) -> torch.Tensor:
        x = batch[k]
        if bs is not None:
            x = x[:bs]
        return x.to(self.device).to(memory_format=torch.contiguous_format).float()

    def get_learned_conditioning(self, txt: Sequence[str]) -> torch.Tensor:
        if self.cond_stage_model is None:
            raise NotImplementedError('no cond_stage_config in the yaml and no cond_stage_model set: '
                                      "put a precomputed [B,77,768] embedding under batch['txt_emb']")
        return self.cond_stage_model(list(txt)).to(self.device).float()

    def get_cond_txt_coding(self, batch: dict, bs: Optional[int] = None) -> torch.Tensor:
        if 'txt_emb' in batch:
            c = batch['txt_emb']
            return (c if bs is None else c[:bs]).to(self.device).float()
        if 'txt_tokens' in batch and self.cond_stage_model is not None:      # ids from an external tokenizer
            tk = batch['txt_tokens']
            return self.cond_stage_model.encode_tokens(tk if bs is None else tk[:bs]).float()
        txt = batch[self.cond_stage_key]
        return self.get_learned_conditioning(txt if bs is None else txt[:bs])

    def get_unconditional_conditioning(self, N: int) -> torch.Tensor:
        if getattr(self, 'uncond_embedding', None) is not None:
            u = self.uncond_embedding.to(self.device).float()
            return u.expand(N, -1, -1).contiguous() if u.shape[0] == 1 else u[:N]
        return self.get_learned_conditioning([''] * N)

    @torch.no_grad()
    def get_input(self, batch: dict, k, bs: Optional[int] = None, *args, **kwargs):
        """-> (None, c) with c_concat = [cat(src_img, ref_img, 1)] (source first) and c_crossattn = [text]."""
        src = self.get_origin_img_input(batch, self.src_img_key, bs)
        ref = self.get_origin_img_input(batch, self.ref_img_key, bs)
        c = {'c_crossattn': [self.get_cond_txt_coding(batch, bs)], 'src_img': src, 'ref_img': ref,
             'c_concat': [torch.cat((src, ref), 1)]}
        return None, c

    def _bind(self, hint: Optional[torch.Tensor], ctx: torch.Tensor, latent_hw) -> MkdEngine:
        eng = self._require_engine()
        extra = (tuple(latent_hw), tuple(self.control_scales), self.only_mid_control)
        if self._bound is None or not self._bound.matches((hint, ctx), extra):
            eng.prepare(hint, ctx, latent_hw=tuple(latent_hw), control_scales=self.control_scales,
                        only_mid_control=self.only_mid_control)
            self._bound = _Held((hint, ctx), extra)
        return eng

    def _bind_cond(self, cond: dict, latent_hw) -> MkdEngine:
        """cat(c_crossattn, 1) / cat(c_concat, 1) of a cond dict (reference diffmk/makeup_diffuse.py:159,165) bound to the engine.
        A list with several entries is concatenated ONCE per distinct set of entries: the key holds the list ELEMENTS (a fresh
        torch.cat result would never match itself and the hint block / K-V caches would be rebuilt every DDIM step)."""
        xs = list(cond['c_crossattn'])
        hs = None if cond.get('c_concat') is None else list(cond['c_concat'])
        if len(xs) == 1 and (hs is None or len(hs) == 1):
            return self._bind(None if hs is None else hs[0], xs[0], latent_hw)
        parts = xs + (hs or [])
        shape = (len(xs), -1 if hs is None else len(hs))
        if self._cat_cache is None or not self._cat_cache[0].matches(parts, shape):
            self._cat_cache = (_Held(parts, shape), torch.cat(xs, 1) if len(xs) > 1 else xs[0],
                               None if hs is None else (torch.cat(hs, 1) if len(hs) > 1 else hs[0]))
        return self._bind(self._cat_cache[2], self._cat_cache[1], latent_hw)

    def reset_conditioning_cache(self) -> None:
        """Drop the prepared-conditioning and CFG-merge caches (and the tensors they hold)."""
        self._bound = None
        self._cfg_cache = None
        self._cat_cache = None

    def cfg_conditioning(self, uncond: dict, cond: dict) -> dict:
        """[uncond; cond] batching (cddim.py:18-38), cached per (uncond, cond) pair so that a step-by-step
        caller does not rebuild — and libmkd does not re-prepare — identical conditioning every step."""
        def flat(c):
            out, names = [], []
            for k in sorted(c):
                v = c[k]
                if isinstance(v, list):
                    out += list(v); names.append((k, len(v)))
                elif isinstance(v, torch.Tensor):
                    out.append(v); names.append((k, -1))
            return out, names
        (tu, nu), (tc, nc) = flat(uncond), flat(cond)
        if self._cfg_cache is None or not self._cfg_cache[0].matches(tu + tc, (tuple(nu), tuple(nc))):
            merged = {}
            for k in cond:
                if isinstance(cond[k], list):
                    merged[k] = [torch.cat([uncond[k][i], cond[k][i]]) for i in range(len(cond[k]))]
                elif isinstance(cond[k], torch.Tensor):
                    merged[k] = torch.cat([uncond[k], cond[k]])
                else:
                    merged[k] = cond[k]
            self._cfg_cache = (_Held(tu + tc, (tuple(nu), tuple(nc))), merged)
        return self._cfg_cache[1]

    # ---- the eps model ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def apply_model(self, x_noisy: torch.Tensor, t: torch.Tensor, cond: dict, return_all: bool = False, *args, **kwargs):
        assert isinstance(cond, dict)
        eng = self._bind_cond(cond, x_noisy.shape[2:])
        eps = eng.eps(x_noisy, t)
        if not return_all:
            return eps
        return eps, self.predict_start_from_noise(x_t=x_noisy, t=t, noise=eps)

    def predict_start_from_noise(self, x_t: torch.Tensor, t: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        a = self.sqrt_recip_alphas_cumprod.to(x_t.device)[t].view(-1, 1, 1, 1)
        b = self.sqrt_recipm1_alphas_cumprod.to(x_t.device)[t].view(-1, 1, 1, 1)
        return a * x_t - b * noise

    # hooks the samplers use to stay on the device ----------------------------------------------------------------
    def ddim_step(self, x, e_c, e_u, scale, a_t, a_prev, sigma_t, s1m_t, noise, temperature, guidance_rescale=0.0):
        return self._require_engine().ddim_step(x, e_c, e_u, scale, a_t, a_prev, sigma_t, s1m_t, noise, temperature,
                                                guidance_rescale=guidance_rescale)

    def q_sample_blend(self, x0, noise, sqrt_ac, sqrt_1m_ac, mask=None, x=None):
        """(sqrt_ac x0 + sqrt_1m_ac noise) * mask + (1 - mask) * x: the masked sampler's blend (mask None: q_sample), same kernel
        arithmetic as the in-library loop"""
        return self._require_engine().q_sample_blend(x0, noise, sqrt_ac, sqrt_1m_ac, mask, x)

    # hipGraph replay of the sampling loop (one captured step, five steps per graph): the configuration bench.py measures.  False: eager
    sample_use_graph = True

    def _bind_guided(self, cond, uncond, scale, latent_hw):
        """(engine bound to cond, or to [uncond; cond] when guidance is on; the cfg_scale to run it with)"""
        cfg_on = not (uncond is None or scale == 1.0)
        c = self.cfg_conditioning(uncond, cond) if cfg_on else cond
        return self._bind_cond(c, latent_hw), float(scale) if cfg_on else 1.0

    # the three loop hooks: bind [uncond; cond] or cond, convert the grid's tables, ask for the trace, call the solver's engine loop
    def _sample_loop(self, solver, x_latent, cond, tables, scale, uncond, log_every_t, guidance_rescale, **kw):
        eng, cfg_scale = self._bind_guided(cond, uncond, scale, x_latent.shape[2:])
        trace = {} if log_every_t is None else dict(log_every_t=int(log_every_t), want_trace=True)
        timesteps, *tables = tables
        return getattr(eng, SOLVERS[solver].loop)(x_latent, [int(v) for v in timesteps], *([float(v) for v in t] for t in tables),
                                                  cfg_scale=cfg_scale, use_graph=bool(self.sample_use_graph),
                                                  guidance_rescale=float(guidance_rescale), **kw, **trace)

    def sample_loop_fast(self, x_latent, cond, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas,
                         unconditional_guidance_scale=1.0, unconditional_conditioning=None, sigmas=None, noise=None, temperature=1.0,
                         x0=None, mask=None, q_sqrt_ac=None, q_sqrt_1m_ac=None, q_noise=None, log_every_t=None, guidance_rescale=0.0):
        """log_every_t not None: (latent, x_inter rows, pred_x0 rows) with the loop's trace (MkdEngine.sample want_trace)"""
        return self._sample_loop('ddim', x_latent, cond, (timesteps, alphas, alphas_prev, sqrt_one_minus_alphas),
                                 unconditional_guidance_scale, unconditional_conditioning, log_every_t, guidance_rescale,
                                 sigmas=None if sigmas is None else [float(v) for v in sigmas], noise=noise, temperature=float(temperature),
                                 x0=x0, mask=mask, q_sqrt_ac=q_sqrt_ac, q_sqrt_1m_ac=q_sqrt_1m_ac, q_noise=q_noise)

    def sample_rows_fast(self, x_latent, cond, rows, solver='ddim', unconditional_conditioning=None, noise=None, temperature=1.0):
        """the whole loop with one request row per sample inside libmkd (mkd_sample_rows; rows: batching.RowTables).  The engine is
        bound to [uncond; cond] exactly when some row's scale is not 1"""
        from ..batching import guided
        g = guided(rows)
        if g and unconditional_conditioning is None:
            raise ValueError('a row with a guidance scale != 1 needs the unconditional conditioning')
        c = self.cfg_conditioning(unconditional_conditioning, cond) if g else cond
        eng = self._bind_cond(c, x_latent.shape[2:])
        return eng.sample_rows(x_latent, rows, solver=solver, noise=noise, temperature=float(temperature), use_graph=bool(self.sample_use_graph))

    def dpmpp_step(self, x, e_c, e_u, scale, coef6, m1=None, m2=None, guidance_rescale=0.0):
        """one DPM-Solver++ multistep update on the device (DPMSolverSampler's per-step loop): (x_prev, x0-prediction), the kernel
        arithmetic of the in-library loop"""
        return self._require_engine().dpmpp_step(x, e_c, e_u, scale, coef6, m1, m2, guidance_rescale=guidance_rescale)

    def sample_loop_dpmpp(self, x_latent, cond, timesteps, alphas, alphas_prev, order=2, lower_order_final=True,
                          unconditional_guidance_scale=1.0, unconditional_conditioning=None, x0=None, mask=None, q_sqrt_ac=None,
                          q_sqrt_1m_ac=None, q_noise=None, log_every_t=None, guidance_rescale=0.0):
        """the whole DPM-Solver++ multistep loop inside libmkd (mkd_sample_dpmpp), on the tables sample_loop_fast takes; log_every_t
        as there"""
        return self._sample_loop('dpmpp', x_latent, cond, (timesteps, alphas, alphas_prev), unconditional_guidance_scale,
                                 unconditional_conditioning, log_every_t, guidance_rescale, order=int(order),
                                 lower_order_final=bool(lower_order_final), x0=x0, mask=mask, q_sqrt_ac=q_sqrt_ac, q_sqrt_1m_ac=q_sqrt_1m_ac,
                                 q_noise=q_noise)

    def unipc_step(self, x, xc_prev, e_c, e_u, scale, coef12, m1=None, m2=None, m3=None, guidance_rescale=0.0):
        """one UniPC step on the device (UniPCSampler's per-step loop): (next predicted latent, corrected latent, x0-prediction), the
        kernel arithmetic of the in-library loop"""
        return self._require_engine().unipc_step(x, xc_prev, e_c, e_u, scale, coef12, m1, m2, m3, guidance_rescale=guidance_rescale)

    def sample_loop_unipc(self, x_latent, cond, timesteps, alphas, alphas_prev, order=2, lower_order_final=True, corrector=True,
                          unconditional_guidance_scale=1.0, unconditional_conditioning=None, log_every_t=None, guidance_rescale=0.0):
        """the whole UniPC predictor-corrector loop inside libmkd (mkd_sample_unipc), on the tables sample_loop_dpmpp takes;
        log_every_t as there"""
        return self._sample_loop('unipc', x_latent, cond, (timesteps, alphas, alphas_prev), unconditional_guidance_scale,
                                 unconditional_conditioning, log_every_t, guidance_rescale, order=int(order),
                                 lower_order_final=bool(lower_order_final), corrector=bool(corrector))

    def latent_mask_from_labels(self, seg: torch.Tensor, classes: Sequence[int] = (0, 11, 12), factor: int = 8,
                                threshold: float = 0.5) -> torch.Tensor:
        """Label map [B,H,W] (uint8) -> latent mask [B,1,H/factor,W/factor] on the device: the area fraction of each block whose label
        is in ``classes``; threshold > 0 makes it binary (fraction >= threshold)."""
        return self._require_engine().latent_mask_from_labels(seg, classes, factor, threshold)

    # ---- sampling drivers ----------------------------------------------------------------------------------------
    # the sampler sample_log runs: 'ddim' (the reference's), 'dpmpp' (DPM-Solver++ multistep of order solver_order on the same grid) or
    # 'unipc' (the UniPC predictor-corrector of order solver_order on that grid; unipc_corrector False: its predictor alone)
    sampler = 'ddim'
    solver_order = 2
    unipc_corrector = True

    def _sampler(self):
        """(the solver record, its sampler class, the solver's own options from the model's attributes) of the ``sampler`` attribute"""
        classes = {'ddim': DDIMSampler, 'dpmpp': DPMSolverSampler, 'unipc': UniPCSampler}
        if self.sampler not in classes:
            raise ValueError(f"sampler must be 'ddim' or 'dpmpp', got {self.sampler!r}")
        solver = SOLVERS[self.sampler]
        return solver, classes[self.sampler], {k: getattr(self, attr) for k, attr in solver.options}

    @torch.no_grad()
    def sample_log(self, cond: dict, batch_size: int, ddim: bool, ddim_steps: int, **kwargs):
        """UPSTREAM ControlLDM.sample_log: latent shape from the hint, x_T ~ N(0, I) unless given.  Upstream ignores ``ddim`` beyond
        picking DDIM; the ``sampler`` attribute is the switch between the two solvers."""
        if not ddim:
            raise NotImplementedError('only the DDIM sampler is on the MakeupDiffuse test path')
        _, _, h, w = cond['c_concat'][0].shape
        shape = (self.channels, h // 8, w // 8)
        _, sampler, options = self._sampler()
        return sampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **options, **kwargs)

    def decode_first_stage(self, z: torch.Tensor) -> torch.Tensor:
        """z / scale_factor -> post_quant_conv -> Decoder (UPSTREAM AutoencoderKL.decode), on the device via mkd_decode."""
        eng = self._require_engine()
        if eng.vae_cfg is None:
            raise NotImplementedError('no first_stage_config in the yaml: the decoder was not configured')
        return eng.decode(z, self.scale_factor)

    # ---- first-stage encoder (opt-in: first_stage_encoder=True) ----------------------------------------------------
    def _require_encoder(self) -> MkdEngine:
        eng = self._require_engine()
        if eng.vae_enc_cfg is None:
            raise NotImplementedError('the first-stage encoder was not configured (construct with first_stage_encoder=True '
                                      'and a first_stage_config)')
        return eng

    @torch.no_grad()
    def encode_first_stage(self, x: torch.Tensor) -> 'DiagonalGaussianPosterior':
        """UPSTREAM AutoencoderKL.encode: Encoder -> quant_conv -> DiagonalGaussianDistribution over the moments (on the device)."""
        _, mom = self._require_encoder().encode(x, 1.0, None, moments=True)
        return DiagonalGaussianPosterior(mom)

    def get_first_stage_encoding(self, encoder_posterior) -> torch.Tensor:
        """UPSTREAM LatentDiffusion.get_first_stage_encoding: scale_factor * posterior.sample() (or * the tensor itself)."""
        if isinstance(encoder_posterior, DiagonalGaussianPosterior):
            z = encoder_posterior.sample()
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    @torch.no_grad()
    def get_z(self, x: torch.Tensor, seeds=None) -> torch.Tensor:
        """reference diffmk/makeup_diffuse.py:37-39 = get_first_stage_encoding(encode_first_stage(x)) as ONE mkd_encode; the noise of
        sample() is drawn as DiagonalGaussianDistribution.sample draws it (torch.randn on the default CPU generator).  ``seeds`` (an int:
        s, s + 1, ...; one per sample; a noise.Seeds): the noise is noise.normal on stream 3 instead, on the device, and no generator
        is advanced."""
        eng = self._require_encoder()
        f = 2 ** (len(eng.vae_enc_cfg.ch_mult) - 1)
        B, _, H, W = x.shape
        if seeds is not None:
            from ..noise import STREAM_POSTERIOR, as_seeds, normal
            noise = normal(as_seeds(seeds, B), (eng.vae_enc_cfg.z_channels, H // f, W // f), stream=STREAM_POSTERIOR, device=self.device)
            return eng.encode(x, self.scale_factor, noise)
        noise = torch.randn((B, eng.vae_enc_cfg.z_channels, H // f, W // f))
        return eng.encode(x, self.scale_factor, noise)

    def decode_latent_code(self, z: torch.Tensor, predict_cids: bool = False, force_not_quantize: bool = False) -> torch.Tensor:
        """reference diffmk/makeups.py:260-262: ``first_stage_model.decode(z / scale_factor)`` (unclamped)."""
        return self.decode_first_stage(z)

    @torch.no_grad()
    def generate_image(self, z: torch.Tensor, format: bool = False) -> torch.Tensor:
        """reference diffmk/makeup_diffuse.py:172-177: decode, clamp to [-1, 1], optionally map to [0, 1]."""
        img = self.decode_first_stage(z).clamp(-1, 1)
        if format:
            img = (img + 1.0) / 2.0
        return img

    @property
    def has_first_stage(self) -> bool:
        return self.engine is not None and self.engine.vae_cfg is not None


class DiagonalGaussianPosterior:
    """UPSTREAM ldm DiagonalGaussianDistribution over device moments [B, 2z, h, w] (mean | logvar), deterministic=False."""

    def __init__(self, parameters: torch.Tensor):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, seeds=None) -> torch.Tensor:
        # drawn on the default CPU generator and moved, as upstream's sample() does: RNG consumption matches
        # seeds (an int: s, s + 1, ...; one per sample; a noise.Seeds): noise.normal on stream 3, no generator is advanced
        if seeds is not None:
            from ..noise import STREAM_POSTERIOR, as_seeds, normal
            nz = normal(as_seeds(seeds, self.mean.shape[0]), tuple(self.mean.shape)[1:], stream=STREAM_POSTERIOR, device=self.parameters.device)
            return self.mean + self.std * nz
        return self.mean + self.std * torch.randn(self.mean.shape).to(device=self.parameters.device)

    def mode(self) -> torch.Tensor:
        return self.mean


class TestDiffuseModel(BaseMakeUpDiffuse):
    """Reference Test* harness classes (diffmk/diffusion_makeup.py:308-411, diffmk/makeup_diffuse.py:413-464):
    adds the sampling settings and ``log_results``' two DDIM passes."""
    __test__ = False          # (pytest: a class named Test*, not a test case)

    def __init__(self, saved_dir: str = './results', model_name: str = 'makeupdiffuse', img_name_key: str = 'img_name',
                 unconditional_guidance_scale: float = 9, ddim_steps: int = 50, ddim_eta: float = 0.0, sample: bool = True,
                 fix_background: bool = False, background_classes: Sequence[int] = (0, 11, 12), background_threshold: float = 0.5,
                 seg_key: str = 'nonmakeup_seg', makeup_score: bool = False, ref_seg_key: str = 'makeup_seg', sampler: str = 'ddim',
                 solver_order: int = 2, unipc_corrector: bool = True, paste_background: bool = False, paste_feather: int = 0, denoise_rows: bool = False,
                 log_every_t: int = 100, guidance_rescale: float = 0.0, face_parser=None, parser_lut=None, parse_size: int = 512,
                 seed: Optional[int] = None, teacher: Optional[str] = None, teacher_feather: int = 2, teacher_strengths=None,
                 teacher_start: Optional[float] = None, teacher_t_min: int = 0, teacher_warp=None, lms_key: str = 'nonmakeup_lms',
                 ref_lms_key: str = 'makeup_lms', teacher_points: Optional[str] = None, teacher_point_dirs: int = 16, *args, **kwargs):
        if teacher not in (None, 'hist'):
            raise ValueError(f"teacher must be None or 'hist' (the histogram-matching pseudo ground truth), got {teacher!r}")
        if teacher_warp is not None and teacher_warp is not False:
            if teacher is None:
                raise ValueError("teacher_warp needs a teacher: construct with teacher='hist'")
            from .. import teacher as _teacher
            _teacher.alpha_rows(teacher_warp, 1)          # (True or a dict of weights in [0, 1], or ValueError)
        if teacher_points is not None or teacher_point_dirs != 16:
            from .. import teacher as _teacher
            _teacher.check_points(teacher_points, teacher_point_dirs)          # (None or 'masks', 8 or 16 directions, or ValueError)
            if teacher_warp is None or teacher_warp is False:
                raise ValueError('teacher_points / teacher_point_dirs choose the control points of the warped term: they need teacher_warp')
            if teacher_points is None:
                raise ValueError("teacher_point_dirs only applies with teacher_points='masks'")
        if teacher is not None or teacher_start is not None:
            from .. import teacher as _teacher
            _teacher.check_feather(teacher_feather)
            if teacher_start is not None:
                if teacher is None:
                    raise ValueError("teacher_start needs a teacher: construct with teacher='hist'")
                _teacher.start_steps(teacher_start, 1)          # (a number in (0, 1], or ValueError)
            if isinstance(teacher_t_min, bool) or int(teacher_t_min) != teacher_t_min or int(teacher_t_min) < 0:
                raise ValueError(f'teacher_t_min must be an integer >= 0, got {teacher_t_min!r}')
        if int(log_every_t) < 1:
            raise ValueError(f'log_every_t must be >= 1, got {log_every_t}')
        if not 0.0 <= float(guidance_rescale) <= 1.0:
            raise ValueError(f'guidance_rescale must lie in [0, 1], got {guidance_rescale}')
        if not 0 <= int(paste_feather) <= 16:
            raise ValueError(f'paste_feather must be 0..16 image pixels, got {paste_feather}')
        if sampler not in SOLVERS:
            raise ValueError(f"sampler must be 'ddim' or 'dpmpp', got {sampler!r}")
        if solver_order not in (1, 2, 3):
            raise ValueError('solver_order must be 1, 2 or 3')
        if int(parse_size) != parse_size or int(parse_size) % 32 or not 64 <= int(parse_size) <= 1024:
            raise ValueError(f'parse_size must be a multiple of 32 in 64..1024, got {parse_size!r}')
        if seed is not None:
            from ..noise import as_seeds
            as_seeds(seed, 1)          # (an integer in 0 .. 2^64 - 1, or ValueError)
        super().__init__(*args, **kwargs)
        # per-sample seeds (noise.py): the default ``seeds=`` of test_step / log_results, transfer_regions, transfer_specs, interpolate
        # and transfer_photos -- sample (or source photo) i of a call gets seed + i, every draw comes from noise.normal and no torch
        # generator is advanced.  None: the torch draws, call for call as before
        self.seed = seed
        # the teacher T of MakeupDiffuse (reference README.md:10, makeup_teacher.py:197-239): 'hist' = EleGANt's pseudo ground truth at
        # warp weight 0, region-wise histogram matching on the device (teacher.pseudo_ground_truth).  log_results then also returns the
        # reference's ground_truth / reconstruction / sample_ddmp rows (diffmk/makeup_diffuse.py:413-464); teacher_start = tau in (0, 1]
        # starts both passes from q_sample(encode(x_p)) and runs only the last k = round(tau S) steps.  None: every call, draw and
        # launch is as before
        self.teacher = teacher
        self.teacher_feather, self.teacher_strengths = int(teacher_feather), teacher_strengths
        self.teacher_start = None if teacher_start is None else float(teacher_start)
        self.teacher_t_min = int(teacher_t_min)
        # teacher_warp (True: the reference's weights skin 0.3 / eye 0.8 / lip 0.1, or a dict over lip / eye / skin): the landmark-warped
        # term of the pseudo ground truth (teacher.warp_blend) from the batch's landmarks batch[lms_key] / batch[ref_lms_key], [B,K,2] in
        # (y, x) pixels of the model-size images.  None / False: the alpha = 0 teacher, call for call as before
        self.teacher_warp = None if teacher_warp is False else teacher_warp
        self.lms_key, self.ref_lms_key = lms_key, ref_lms_key
        # teacher_points='masks': the control points of the warped term come from the region masks (teacher.region_points with
        # teacher_point_dirs directions) and the spline is solved on the device, so the batch needs no landmark keys and
        # transfer_photos(teacher_start=) takes teacher_warp.  None: the landmarks above, call for call as before
        self.teacher_points, self.teacher_point_dirs = teacher_points, int(teacher_point_dirs)
        # label maps from the images themselves (face_parser.FaceParser, or anything with its parse()): a batch that lacks seg_key /
        # ref_seg_key gets them from the source / reference image parsed at parse_size; label maps the caller brings always win.
        # None: every path is as before (a missing label map is a KeyError)
        from ..face_parser import LUT_SEG
        self.face_parser = face_parser
        self.parser_lut = tuple(LUT_SEG if parser_lut is None else parser_lut)
        self.parse_size = int(parse_size)
        # log_results' sampler: 'dpmpp' runs both passes on DPM-Solver++ multistep (ddim_steps is then its number of evaluations)
        # 'unipc': the UniPC predictor-corrector at the same number of evaluations (unipc_corrector False: the predictor alone)
        self.sampler, self.solver_order = sampler, int(solver_order)
        self.unipc_corrector = bool(unipc_corrector)
        # makeup score of every decoded sample (makeup_score.transfer_score): off by default, then log_results is unchanged
        self.makeup_score = bool(makeup_score)
        self.ref_seg_key = ref_seg_key
        # background-preserving transfer (reference Fixbackground classes: background 0, teeth 11, hair 12): both sampling passes
        # keep the source's latent where the label map says so (DDIMSampler mask / x0)
        self.fix_background = bool(fix_background)
        self.background_classes = tuple(int(c) for c in background_classes)
        self.background_threshold = float(background_threshold)
        self.seg_key = seg_key
        # pixel-space paste after the decode (reference Fixbackground.get_target): every decoded sample keeps the SOURCE's pixels over
        # background_classes of batch[seg_key], mixed over paste_feather image pixels on both sides of the boundary (0: the reference's hard
        # mask).  Independent of fix_background (needs neither the encoder nor masked sampling); off: log_results is unchanged
        self.paste_background = bool(paste_background)
        self.paste_feather = int(paste_feather)
        # denoise rows (reference log_images plot_denoise_rows / _get_denoise_row_from_list): log_results also returns the decoded pred_x0
        # list of each pass, logged every log_every_t table entries by the in-library loop's trace.  Off: log_results is unchanged
        self.denoise_rows = bool(denoise_rows)
        self.log_every_t = int(log_every_t)
        # guidance rescale phi of the guided pass(es) (per-sample std ratio inside every step); 0: off, today's path
        self.guidance_rescale = float(guidance_rescale)
        self.unconditional_guidance_scale = unconditional_guidance_scale
        self.ddim_steps, self.ddim_eta, self.sample = ddim_steps, ddim_eta, sample
        self.saved_dir, self.model_name, self.img_name_key = saved_dir, model_name, img_name_key
        self.clamp = True
        self.rescale = True
        self.save_images = True                    # save_local after every test_step, as the reference does
        self.test_pairs: list = []
        self.test_pairs_file = 'test_0412_pairs.txt'

    def _seeds(self, seeds, n: int):
        """the noise.Seeds of a call over n samples: its ``seeds=``, else the model's ``seed``, else None (the torch draws)"""
        if seeds is None:
            seeds = self.seed
        if seeds is None:
            return None
        from ..noise import as_seeds
        return as_seeds(seeds, n)

    def _start_latent(self, x_T, sd, n: int, h: int, w: int) -> torch.Tensor:
        """x_T as given; else noise.normal on stream 0 with seeds; else a torch draw on the device generator"""
        if x_T is not None:
            return x_T.to(self.device)
        if sd is not None:
            from ..noise import STREAM_START, normal
            return normal(sd, (self.channels, h, w), stream=STREAM_START, device=self.device)
        return torch.randn(n, self.channels, h, w, device=self.device)

    def on_test_epoch_start(self) -> None:
        self.eval()
        self.test_pairs = []

    def on_test_batch_end(self, outputs=None, batch=None, batch_idx: int = 0, dataloader_idx: int = 0) -> None:
        """'num-num nonmakeup makeup' bookkeeping file (diffusion_makeup.py:327-331), rewritten after every batch."""
        with open(self.test_pairs_file, 'w') as f:
            for tp in self.test_pairs:
                f.write('%s %s %s\n' % (tp[0], tp[1], tp[2]))

    @torch.no_grad()
    def parse_images(self, img01: torch.Tensor) -> torch.Tensor:
        """label maps uint8 [B,H,W] of images [B,3,H,W] in [0,1] from the attached face parser: parsed at parse_size x parse_size (the
        reference parses at 512 x 512, diffdata/preprocessing.py:151-157; images of another size are resized with antialiased bilinear
        interpolation first), the label map brought to the images' size by the head's nearest rule, classes remapped by parser_lut"""
        if self.face_parser is None:
            raise ValueError('no face parser is attached (face_parser=...)')
        H, W = int(img01.shape[-2]), int(img01.shape[-1])
        S = self.parse_size
        x = img01.float()
        if (H, W) != (S, S):
            x = torch.nn.functional.interpolate(x, size=(S, S), mode='bilinear', align_corners=False, antialias=True).clamp(0.0, 1.0)
        return self.face_parser.parse(x, out_size=(H, W), lut=self.parser_lut)

    def _fill_segs(self, batch: dict, ref: bool = False) -> None:
        """with a face parser attached: batch[seg_key] (and batch[ref_seg_key] when ``ref``) from the batch's own images where the
        batch does not bring them.  The maps are written INTO the caller's dict, on purpose: log_results, paste_source, background_latents,
        makeup_hist and transfer_regions all pass through here, and a batch parsed once is not parsed again by the next of them (nor by
        the caller's next call on the same batch).  Without a parser nothing happens and the callers' KeyErrors stand."""
        if self.face_parser is None:
            return
        for seg_k, img_k in ((self.seg_key, self.src_img_key),) + (((self.ref_seg_key, self.ref_img_key),) if ref else ()):
            if seg_k not in batch and img_k in batch:
                batch[seg_k] = self.parse_images(self.get_origin_img_input(batch, img_k))

    @torch.no_grad()
    def log_results(self, batch: dict, batch_idx: int, x_T: Optional[torch.Tensor] = None, seeds=None) -> Dict[str, torch.Tensor]:
        """The sampler calls of reference log_results (:391-410): a plain 50-step pass and a CFG pass whose
        unconditional branch keeps the SAME hint (uc_cat = c_cat, :401).  Returns latents (and decoded images
        once a first_stage_model is attached).  With teacher='hist' also the reference's teacher rows (_teacher_rows) and, with
        teacher_start, both passes start from the diffused teacher latent and run k steps (_teacher_start).  With a face parser attached, label
        maps the batch lacks are added to ``batch`` (_fill_segs).  ``seeds`` (default: the model's ``seed``; one per pair, or an int s
        for s, s + 1, ...): every draw of both passes and of fix_background's encoder comes from noise.normal; both passes start from the
        same seeded x_T, as they do from a given ``x_T``."""
        use_ddim = self.ddim_steps is not None
        log: Dict[str, torch.Tensor] = {}
        self._check_unipc_masked()
        if self.teacher is not None:
            self._check_teacher(batch, x_T)
        if self.fix_background or self.paste_background or self.makeup_score:
            self._fill_segs(batch, ref=self.makeup_score)
        _, c = self.get_input(batch, self.first_stage_key)
        c_cat, c_txt = c['c_concat'][0], c['c_crossattn'][0]
        src, ref = torch.chunk(c_cat, 2, dim=1)
        log['control_src'] = src * 2.0 - 1.0
        log['control_ref'] = ref * 2.0 - 1.0
        names = batch.get(self.img_name_key)
        if names is not None:                      # :379-384
            for i, nm in enumerate(names):
                self.test_pairs.append(['%04d-%d' % (batch_idx, i + 1), 'non-makeup/%s.png' % nm.split('&')[0],
                                        'makeup/%s.png' % nm.split('&')[1]])
        b = c_cat.shape[0]
        extra = {} if x_T is None else {'x_T': x_T}
        sd = self._seeds(seeds, b)
        if sd is not None:
            extra['seeds'] = sd
        if self.fix_background:
            x0, mask = self.background_latents(batch, c['src_img'], seeds=sd)
            extra.update(x0=x0, mask=mask)
            log['mask_latent'] = mask
        if self.paste_background:
            self._check_paste(batch, 'paste_background')
        cond = {'c_concat': [c_cat], 'c_crossattn': [c_txt]}
        if self.denoise_rows:
            extra['log_every_t'] = self.log_every_t
        sample_log = self.sample_log
        if self.teacher is not None:
            z_p = self._teacher_rows(log, batch, src, ref, c['ref_img'], cond, sd)
            if self.teacher_start is not None:
                sample_log = self._teacher_start(z_p if z_p is not None else self.get_z(log['ground_truth'], seeds=sd), sd)
        if self.sample:
            samples, inter = sample_log(cond=cond, batch_size=b, ddim=use_ddim, ddim_steps=self.ddim_steps,
                                        eta=self.ddim_eta, **extra)
            log['samples_latent'] = samples
            if self.denoise_rows:
                self._log_denoise_row(log, 'denoise_row', inter['pred_x0'])
            if self.has_first_stage:
                log['samples'] = self.decode_first_stage(samples)
                if self.paste_background:
                    log['samples'], log['mask_pixel'] = self.paste_source(batch, log['samples'], log['control_src'])
                if self.makeup_score:
                    log['makeup_hist'] = self.makeup_hist(batch, log['samples'], c['ref_img'])
        if self.unconditional_guidance_scale > 1.0:
            uc_full = {'c_concat': [c_cat], 'c_crossattn': [self.get_unconditional_conditioning(b)]}
            if self.guidance_rescale != 0.0:
                extra['guidance_rescale'] = self.guidance_rescale
            samples_cfg, inter = sample_log(cond=cond, batch_size=b, ddim=use_ddim, ddim_steps=self.ddim_steps,
                                            eta=self.ddim_eta, unconditional_guidance_scale=self.unconditional_guidance_scale,
                                            unconditional_conditioning=uc_full, **extra)
            name = f'samples_cfg_scale_{self.unconditional_guidance_scale:.2f}'
            log[name + '_latent'] = samples_cfg
            if self.denoise_rows:
                self._log_denoise_row(log, f'denoise_row_cfg_scale_{self.unconditional_guidance_scale:.2f}', inter['pred_x0'])
            if self.has_first_stage:
                log[name] = self.decode_first_stage(samples_cfg)
                if self.paste_background:
                    log[name], log['mask_pixel'] = self.paste_source(batch, log[name], log['control_src'])
                if self.makeup_score:
                    log[f'makeup_hist_cfg_scale_{self.unconditional_guidance_scale:.2f}'] = self.makeup_hist(batch, log[name], c['ref_img'])
        return log

    # ---- the teacher (opt-in: teacher='hist') ---------------------------------------------------------------------------------------
    def _check_teacher(self, batch: dict, x_T) -> None:
        """what the teacher options need and what they are not combined with; raised before anything is enqueued"""
        if self.face_parser is None:
            for k in (self.seg_key, self.ref_seg_key):
                if k not in batch:
                    raise ValueError(f"teacher='hist' needs the label maps of the source and of the reference: the batch has none under "
                                     f"'{k}' and no face parser is attached")
        if self.teacher_warp is not None and self.teacher_points is None:
            for k in (self.lms_key, self.ref_lms_key):
                if k not in batch:
                    raise ValueError(f"teacher_warp needs the landmarks of the source and of the reference: the batch has none under '{k}'")
        if not 0 <= self.teacher_t_min < self.num_timesteps:
            raise ValueError(f'teacher_t_min must lie in 0 .. {self.num_timesteps - 1}, got {self.teacher_t_min}')
        if self.teacher_start is not None:
            if self.denoise_rows:
                raise ValueError('teacher_start is not combined with denoise_rows')
            self._check_teacher_start(x_T, self.guidance_rescale)

    def _refuse_teacher_start(self, what: str) -> None:
        """teacher_start acts in log_results / test_step and, as a keyword, in transfer_photos: every other sampling entry refuses a
        model that carries it rather than running full passes without saying so"""
        if self.teacher_start is not None:
            raise ValueError(f'teacher_start is not combined with {what}')

    def _check_teacher_start(self, x_T, phi) -> None:
        if x_T is not None:
            raise ValueError('teacher_start with a given x_T: the start latent is the diffused teacher image, x_T would be ignored')
        for on, what in ((self.fix_background, 'fix_background (a masked decode does not exist)'),
                         (phi != 0.0 and float(self.unconditional_guidance_scale) > 1.0, "guidance_rescale (the solvers' decode does not carry it)"),
                         (float(self.ddim_eta or 0.0) != 0.0, 'ddim_eta != 0 (the teacher-started pass is deterministic after its start)')):
            if on:
                raise ValueError(f'teacher_start is not combined with {what}')
        if not self.ddim_steps or int(self.ddim_steps) < 1:
            raise ValueError('teacher_start needs ddim_steps >= 1')
        self._sampler()
        self._require_encoder()

    def pseudo_ground_truth(self, batch: dict, src01: torch.Tensor, ref01: torch.Tensor) -> torch.Tensor:
        """x_p in [0, 1] of the pairs (src01, ref01) under batch[seg_key] / batch[ref_seg_key] (parsed from the batch's images where a
        face parser is attached and the batch lacks them): teacher.pseudo_ground_truth with the model's teacher_feather / _strengths and,
        with teacher_warp, the landmarks batch[lms_key] / batch[ref_lms_key] (teacher_points='masks': the control points of the masks)"""
        from .. import teacher
        self._fill_segs(batch, ref=True)
        for k in (self.seg_key, self.ref_seg_key):
            if k not in batch:
                raise ValueError(f"teacher='hist' needs the label maps of the source and of the reference: the batch has none under '{k}'")
        warp = self._mask_points_warp()
        if self.teacher_warp is not None and not warp:
            for k in (self.lms_key, self.ref_lms_key):
                if k not in batch:
                    raise ValueError(f"teacher_warp needs the landmarks of the source and of the reference: the batch has none under '{k}'")
            warp = dict(lms_src=batch[self.lms_key], lms_ref=batch[self.ref_lms_key], warp=self.teacher_warp)
        return teacher.pseudo_ground_truth(src01, ref01, batch[self.seg_key], batch[self.ref_seg_key], strengths=self.teacher_strengths,
                                           feather=self.teacher_feather, **warp)[0]

    def _mask_points_warp(self) -> dict:
        """teacher.pseudo_ground_truth's keywords of the warped term with control points from the masks; {} unless the model has both
        teacher_warp and teacher_points='masks'"""
        if self.teacher_warp is None or self.teacher_points is None:
            return {}
        return dict(warp=self.teacher_warp, points=self.teacher_points, point_dirs=self.teacher_point_dirs)

    def _teacher_rows(self, log: dict, batch: dict, src01, ref01, ref_img, cond: dict, sd):
        """The rows reference log_results writes beside the samples (diffmk/makeup_diffuse.py:419-442): ground_truth = 2 x_p - 1; with an
        encoder and a decoder reconstruction = decode(get_z(ground_truth)) and sample_ddmp = the decoded x0 prediction of ONE apply_model
        call on q_sample(z, t), t_b in [teacher_t_min, T); with makeup_score the score of x_p.  Without seeds the draws are the
        reference's, in its order: get_z's posterior noise, torch.randint for t, torch.randn_like for the noise.  With seeds t_b =
        noise.teacher_timesteps(seed_b, sub_b) and the noise is noise.normal on STREAM_TEACHER, row 0.  Returns z (or None)."""
        x_p = self.pseudo_ground_truth(batch, src01, ref01)
        log['ground_truth'] = x_p * 2.0 - 1.0
        if self.makeup_score:
            log['makeup_hist_teacher'] = self.makeup_hist(batch, log['ground_truth'], ref_img)
        if not (self.has_first_stage and self._require_engine().vae_enc_cfg is not None):
            return None
        z = self.get_z(log['ground_truth'], seeds=sd)
        log['reconstruction'] = self.decode_first_stage(z)
        if sd is not None:
            from ..noise import STREAM_TEACHER, normal, teacher_timesteps
            t = torch.tensor(teacher_timesteps(sd, self.teacher_t_min, self.num_timesteps), dtype=torch.long).to(self.device)
            nz = normal(sd, tuple(z.shape)[1:], stream=STREAM_TEACHER, device=self.device)
        else:
            t = torch.randint(self.teacher_t_min, self.num_timesteps, (z.shape[0],), device=self.device).long()
            nz = torch.randn_like(z)
        x_noisy = (self.sqrt_alphas_cumprod.to(self.device)[t].view(-1, 1, 1, 1) * z
                   + self.sqrt_one_minus_alphas_cumprod.to(self.device)[t].view(-1, 1, 1, 1) * nz)          # UPSTREAM DDPM.q_sample
        _, x_recon = self.apply_model(x_noisy, t, cond, return_all=True)
        log['sample_ddmp'] = self.decode_first_stage(x_recon)
        return z

    def _teacher_start(self, z_p: torch.Tensor, sd, tau=None):
        """sample_log's stand-in of a teacher-started pass: k = teacher.start_steps(tau or teacher_start, ddim_steps); the start latent is
        stochastic_encode(z_p, k - 1) on the sampler's schedule of ddim_steps (seeded: stream 2 row 0; else one randn_like), drawn ONCE
        and shared by both passes as x_T is; each pass is the solver's decode(x, cond, t_start=k): k evaluations instead of ddim_steps"""
        from .. import teacher
        solver, cls, options = self._sampler()
        k = teacher.start_steps(self.teacher_start if tau is None else tau, self.ddim_steps)
        smp = cls(self)
        if solver.name == 'ddim':
            smp.make_schedule(ddim_num_steps=self.ddim_steps, ddim_eta=0.0, verbose=False)
        else:
            smp.make_schedule(self.ddim_steps)
        x_start = getattr(smp, '_ddim', smp).stochastic_encode(z_p, k - 1, **({} if sd is None else {'seeds': sd}))

        def sample_log(cond, unconditional_guidance_scale=1.0, unconditional_conditioning=None, **rest):
            # sample_log's own keywords that a decode does not take: the batch and the grid are the start latent's, eta is refused unless
            # 0, the seeds went into the start.  Anything else (x_T, mask / x0, log_every_t, guidance_rescale, ...) must not get here
            unknown = sorted(set(rest) - {'batch_size', 'ddim', 'ddim_steps', 'eta', 'seeds'})
            if unknown or rest.get('eta') not in (None, 0, 0.0):
                raise TypeError(f'a teacher-started pass does not carry {unknown or "eta"}')
            return smp.decode(x_start, cond, k, unconditional_guidance_scale=unconditional_guidance_scale,
                              unconditional_conditioning=unconditional_conditioning, **options), None
        return sample_log

    @torch.no_grad()
    def transfer_specs(self, batch: dict, specs, x_T: Optional[torch.Tensor] = None, seeds=None) -> Dict[str, torch.Tensor]:
        """One ``batching.SampleSpec`` per pair of the batch (steps, eta, guidance, t_start, order), sampled together: requests that
        differ in step count, strength, guidance scale or eta share one batch.  As in log_results the conditioning is the pair's hint
        and text, and a guided sample's unconditional branch keeps the SAME hint.  One pass per prepared-batch form: the samples whose
        guidance is 1 run as one per-sample loop on the batch-B conditioning, the others as one on [uncond; cond]; each pass is one
        loop of its longest member.  The ``sampler`` attribute picks the solver.  Returns samples_latent (rows in batch order) and,
        with a first stage, the decoded samples.  ``seeds`` (default: the model's ``seed``): one per pair, beside the specs; each pass
        gets its members' seeds, so a pair's noise does not depend on which pass it runs in."""
        from ..batching import SampleSpec
        self._refuse_teacher_start('transfer_specs (a SampleSpec carries its own t_start: compose it with teacher.pseudo_ground_truth '
                                   'and stochastic_encode)')
        solver = SOLVERS.get(self.sampler)
        if solver is not None and solver.rows_id is None:
            self._sampler()[1](self).sample_specs()          # (NotImplementedError: the per-sample loop runs DDIM and DPM-Solver++ only)
        specs = list(specs)
        _, c = self.get_input(batch, self.first_stage_key)
        c_cat, c_txt = c['c_concat'][0], c['c_crossattn'][0]
        b = c_cat.shape[0]
        if len(specs) != b or not all(isinstance(s, SampleSpec) for s in specs):
            raise ValueError(f'transfer_specs: one SampleSpec per pair is needed ({len(specs)} for a batch of {b})')
        smp = self._sampler()[1](self)
        h, w = c_cat.shape[2] // 8, c_cat.shape[3] // 8
        sd = self._seeds(seeds, b)
        x_T = self._start_latent(x_T, sd, b, h, w)
        if tuple(x_T.shape) != (b, self.channels, h, w):
            raise ValueError(f'transfer_specs: x_T must be {(b, self.channels, h, w)}, got {tuple(x_T.shape)}')
        lat = torch.empty_like(x_T)
        for want_guided in (False, True):
            idx = [i for i, s in enumerate(specs) if (float(s.guidance) != 1.0) == want_guided]
            if not idx:
                continue
            sel = torch.as_tensor(idx, device=self.device)
            cond = {'c_concat': [c_cat[sel].contiguous()], 'c_crossattn': [c_txt[sel].contiguous()]}
            uc = None
            if want_guided:
                uc = {'c_concat': cond['c_concat'], 'c_crossattn': [self.get_unconditional_conditioning(len(idx))]}
            lat[sel] = smp.sample_specs([specs[i] for i in idx], (self.channels, h, w), cond, x_T=x_T[sel].contiguous(),
                                        unconditional_conditioning=uc, **({} if sd is None else {'seeds': sd.take(idx)}))
        out = {'samples_latent': lat}
        if self.has_first_stage:
            out['samples'] = self.decode_first_stage(lat)
        return out

    def _log_denoise_row(self, log: dict, name: str, pred_x0: list) -> None:
        """reference _get_denoise_row_from_list before its make_grid: the pred_x0 list of a pass (x_T first, then one entry per logged
        step) stacked 'n b c h w -> (b n) c h w', samples as rows and list entries as columns: entry [i * n + j] is sample i at list
        entry j.  name_latent holds the latents, name their decode_first_stage images (each list entry decoded as one batch)."""
        lat = torch.stack(list(pred_x0), dim=1)
        log[name + '_latent'] = lat.reshape(-1, *lat.shape[2:])
        if self.has_first_stage:
            img = torch.stack([self.decode_first_stage(z) for z in pred_x0], dim=1)
            log[name] = img.reshape(-1, *img.shape[2:])

    @torch.no_grad()
    def makeup_hist(self, batch: dict, sample: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
        """makeup_score: [B,4] = lip, skin, eye_left, eye_right histogram-matching distance of a decoded sample ([-1,1]) against the
        makeup reference ([0,1]) under batch[seg_key] / batch[ref_seg_key] (reference criterionHis, diffmk/makeups.py:232-245)."""
        from .. import makeup_score as ms
        self._fill_segs(batch, ref=True)
        for k in (self.seg_key, self.ref_seg_key):
            if k not in batch:
                raise KeyError(f"makeup_score: the batch has no label map under '{k}'")
        img = ((sample.float() + 1.0) / 2.0).clamp(0, 1)
        return ms.transfer_score(img, ref, batch[self.seg_key], batch[self.ref_seg_key])

    def _check_unipc_masked(self) -> None:
        """fix_background samples with a mask; the UniPC solver has no masked form (UniPCSampler.sample).  Raised before the encoder,
        the parser or a sampler has enqueued anything"""
        solver = SOLVERS.get(self.sampler)
        if self.fix_background and solver is not None and not solver.masked:
            raise NotImplementedError(f'{self._sampler()[1].__name__}: masked sampling (mask / x0) is not defined for this solver: '
                                      "fix_background needs sampler='ddim' or 'dpmpp'")

    def _check_paste(self, batch: dict, what: str) -> None:
        """what a pixel-space paste needs, checked before anything is sampled"""
        if not self.has_first_stage:
            raise ValueError(f'{what} pastes decoded images: it needs a first stage (first_stage_config)')
        self._fill_segs(batch)
        if self.seg_key not in batch:
            raise KeyError(f"{what}: the batch has no label map under '{self.seg_key}'")

    @torch.no_grad()
    def paste_source(self, batch: dict, image: torch.Tensor, src: torch.Tensor):
        """paste_background: (the decoded ``image`` with the pixels of ``src`` ([-1, 1]) over background_classes of batch[seg_key], feathered
        by paste_feather; the keep weights [B,1,H,W]) -- one mkd_paste_background launch"""
        self._check_paste(batch, 'paste_background')
        return self._require_engine().paste_background(image, src, seg=batch[self.seg_key], classes=self.background_classes,
                                                       feather=self.paste_feather, return_alpha=True)

    @torch.no_grad()
    def background_latents(self, batch: dict, src: torch.Tensor, seeds=None):
        """fix_background: x0 = get_z(src * 2 - 1) and the latent mask of batch[seg_key] over background_classes.  seeds: get_z's."""
        if not self.first_stage_encoder:
            raise ValueError('fix_background needs the first-stage encoder: construct with first_stage_encoder=True')
        self._fill_segs(batch)
        if self.seg_key not in batch:
            raise KeyError(f"fix_background: the batch has no label map under '{self.seg_key}'")
        seg = batch[self.seg_key]
        lw = src.shape[-1] // 8
        if lw <= 0 or seg.shape[-1] % lw:
            raise ValueError(f'fix_background: label map width {seg.shape[-1]} is not a multiple of the latent width {lw}')
        mask = self.latent_mask_from_labels(seg, self.background_classes, seg.shape[-1] // lw, self.background_threshold)
        x0 = self.get_z(src * 2.0 - 1.0, **({} if seeds is None else {'seeds': seeds}))
        return x0, mask

    @torch.no_grad()
    def interpolate(self, batch: dict, alphas, x_T: Optional[torch.Tensor] = None, ref2_key: str = 'ref_img2',
                    unconditional_guidance_scale: float = 1.0, seeds=None) -> Dict[str, torch.Tensor]:
        """Makeup interpolation between two references (README.md:23-25 shows the figure; the reference has no code, so the
        definition is this build's: the ControlNet hint embeddings E(src||ref1), E(src||ref2) are blended per sample with
        weight alpha before the 50-step loop).  batch holds src_img, ref_img, `ref2_key`, txt_emb for
        N pairs; every pair is sampled at every alpha -> latents [N*len(alphas), 4, h, w] ordered pair-major.  ``seeds`` (default: the
        model's ``seed``): one per PAIR; without ``x_T`` the pair's start noise is noise.normal on stream 0, shared by its alphas."""
        self._refuse_teacher_start('interpolate (two references: the teacher image of one pair does not exist)')
        src = self.get_origin_img_input(batch, self.src_img_key)
        r1 = self.get_origin_img_input(batch, self.ref_img_key)
        r2 = self.get_origin_img_input(batch, ref2_key)
        ctx = self.get_cond_txt_coding(batch)
        A = torch.as_tensor(list(alphas), dtype=torch.float32)
        n, k = src.shape[0], A.numel()
        rep = lambda t: t.repeat_interleave(k, 0)
        h1, h2 = rep(torch.cat((src, r1), 1)), rep(torch.cat((src, r2), 1))
        ctxr, al = rep(ctx), A.repeat(n).to(self.device)
        eng = self._require_engine()
        h, w = src.shape[2] // 8, src.shape[3] // 8
        x_T = rep(self._start_latent(x_T, self._seeds(seeds, n), n, h, w))           # the same start noise for every alpha of a pair
        if self.paste_background:
            self._check_paste(batch, 'paste_background')
        sch = self.schedule
        sch.make_ddim(self.ddim_steps, ddim_eta=0.0)
        if unconditional_guidance_scale != 1.0:
            u = self.get_unconditional_conditioning(n * k)
            eng.prepare(torch.cat([h1, h1]), torch.cat([u, ctxr]), hint2=torch.cat([h2, h2]), alpha=torch.cat([al, al]),
                        control_scales=self.control_scales, only_mid_control=self.only_mid_control)
        else:
            eng.prepare(h1, ctxr, hint2=h2, alpha=al, control_scales=self.control_scales, only_mid_control=self.only_mid_control)
        self.reset_conditioning_cache()
        lat = eng.sample(x_T, sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas,
                         cfg_scale=float(unconditional_guidance_scale), use_graph=True)
        out = {'samples_latent': lat, 'alpha': al}
        if self.has_first_stage:
            out['samples'] = self.decode_first_stage(lat)
            if self.paste_background:          # every alpha of a pair keeps that pair's source
                out['samples'], out['mask_pixel'] = self._require_engine().paste_background(
                    out['samples'], rep(src) * 2.0 - 1.0, seg=rep(batch[self.seg_key].to(self.device)), classes=self.background_classes,
                    feather=self.paste_feather, return_alpha=True)
        return out

    @torch.no_grad()
    def transfer_regions(self, batch: dict, refs: Dict[str, str], strengths: Optional[dict] = None, base: str = 'ref', feather: int = 1,
                         x_T: Optional[torch.Tensor] = None, unconditional_guidance_scale: float = 1.0,
                         paste_outside: bool = False, guidance_rescale: Optional[float] = None, seeds=None) -> Dict[str, torch.Tensor]:
        """Region-wise makeup transfer from several references (partial transfer as SCGAN / EleGANt / PSGAN offer it; the reference
        has no code for it, so the definition is this build's): ``refs`` maps the user regions 'eye', 'lip', 'skin' to the
        batch keys of their reference images; the ControlNet hint embeddings E(src||ref_r) are blended PER LATENT PIXEL with the
        weights that regions.region_weights_from_seg takes from batch[seg_key] (priority eye > lip > skin, ``feather`` latent pixels
        of box smoothing, ``strengths`` {region: a number or one per sample}, default 1).  Pixels of no region, and what a strength
        below 1 leaves, follow the base hint: src||ref_img (base='ref') or src||src (base='source': towards no makeup).  Runs the
        ``sampler`` attribute's solver for ddim_steps from x_T.  Returns samples_latent, weights [B, 1 + regions, h, w] (plane 0 the
        base, then the regions in priority order) and, with a first-stage decoder, samples.  With the paste_background option the samples
        keep the source's pixels over background_classes (mask_pixel holds the weights); ``paste_outside`` (base='source' only) then also
        pastes the source over everything that belongs to NONE of the chosen regions, feathered by paste_feather (weights: mask_outside),
        so that "lips only" leaves the rest of the face alone.  ``guidance_rescale`` (default: the model's setting) is the phi of the
        guided pass, engaged with unconditional_guidance_scale != 1 and phi > 0.  ``seeds`` (default: the model's ``seed``): one per pair;
        without ``x_T`` the start noise is noise.normal on stream 0 -- the only draw of this deterministic pass."""
        self._refuse_teacher_start('transfer_regions (several references: the teacher image of one pair does not exist)')
        from .. import regions as rg
        phi = float(self.guidance_rescale if guidance_rescale is None else guidance_rescale)
        if not 0.0 <= phi <= 1.0:
            raise ValueError(f'guidance_rescale must lie in [0, 1], got {phi}')
        regs = rg.ordered(refs)
        if base not in ('ref', 'source'):
            raise ValueError(f"base must be 'ref' or 'source', got {base!r}")
        if paste_outside and base != 'source':
            raise ValueError("paste_outside keeps the source outside the chosen regions: it needs base='source'")
        if not 0 <= int(feather) <= rg.MAX_FEATHER:
            raise ValueError(f'feather must be 0..{rg.MAX_FEATHER} latent pixels, got {feather}')
        self._fill_segs(batch)
        if self.seg_key not in batch:
            raise KeyError(f"transfer_regions: the batch has no label map under '{self.seg_key}'")
        if paste_outside or self.paste_background:
            self._check_paste(batch, 'paste_outside' if paste_outside else 'paste_background')
        for r in regs:
            if refs[r] not in batch:
                raise KeyError(f"transfer_regions: the batch has no reference image under '{refs[r]}' (region '{r}')")
        n = int(batch[self.src_img_key].shape[0])
        rg.strength_rows(strengths, regs, n)                  # (validates before anything reaches the device)
        sd = self._seeds(seeds, n)
        eng = self._require_engine()
        src = self.get_origin_img_input(batch, self.src_img_key)
        base_img = src if base == 'source' else self.get_origin_img_input(batch, self.ref_img_key)
        hints = [torch.cat((src, base_img), 1)] + [torch.cat((src, self.get_origin_img_input(batch, refs[r])), 1) for r in regs]
        ctx = self.get_cond_txt_coding(batch)
        h, w = src.shape[2] // 8, src.shape[3] // 8
        seg = batch[self.seg_key]
        seg = rg.ms.label_map(seg)
        factor = seg.shape[-1] // w if w > 0 else 0
        if factor < 1 or (seg.shape[-2], seg.shape[-1]) != (factor * h, factor * w):
            raise ValueError(f'transfer_regions: label map {tuple(seg.shape[-2:])} is not a multiple of the latent {(h, w)}')
        weights = rg.region_weights_from_seg(seg.to(self.device), regs, factor, int(feather), strengths)
        x_T = self._start_latent(x_T, sd, n, h, w)
        scale = float(unconditional_guidance_scale)
        if scale != 1.0:          # [uncond; cond] with the SAME hints and weights in both halves (log_results: uc_cat = c_cat)
            u = self.get_unconditional_conditioning(n)
            eng.prepare_regions([torch.cat([t, t]) for t in hints], torch.cat([weights, weights]), torch.cat([u, ctx]),
                                control_scales=self.control_scales, only_mid_control=self.only_mid_control)
        else:
            eng.prepare_regions(hints, weights, ctx, control_scales=self.control_scales, only_mid_control=self.only_mid_control)
        self.reset_conditioning_cache()
        sch = self.schedule
        sch.make_ddim(self.ddim_steps, ddim_eta=0.0)
        ts = [int(v) for v in sch.ddim_timesteps]
        a, ap = [float(v) for v in sch.ddim_alphas], [float(v) for v in sch.ddim_alphas_prev]
        solver, _, options = self._sampler()
        tables = (a, ap, [float(v) for v in sch.ddim_sqrt_one_minus_alphas]) if solver.name == 'ddim' else (a, ap)
        lat = getattr(eng, solver.loop)(x_T, ts, *tables, cfg_scale=scale, use_graph=bool(self.sample_use_graph), guidance_rescale=phi,
                                        **options)
        out = {'samples_latent': lat, 'weights': weights}
        if self.has_first_stage:
            out['samples'] = self.decode_first_stage(lat)
            if self.paste_background:
                out['samples'], out['mask_pixel'] = self.paste_source(batch, out['samples'], src * 2.0 - 1.0)
            if paste_outside:                  # a 0/1 map is itself a label map: the same launch with classes = (1,)
                keep = 1 - rg.user_region_masks(seg.to(self.device), regs).amax(0)
                out['samples'], out['mask_outside'] = eng.paste_background(out['samples'], src * 2.0 - 1.0, seg=keep, classes=(1,),
                                                                           feather=self.paste_feather, return_alpha=True)
        return out

    def _photo_pass(self, src_photos, ref_photos, src_regions, ref_regions, src_segs, x_T, size, batch, phi, seeds=None, teacher=None,
                    ref_segs=None):
        """the single pass of transfer_photos for one batch of (photo, region) pairs on the device: crop-resize both, sample, decode,
        paste_source -> (the decoded images [n,3,size,size], the source crops img01 the paste needs).  A region is a box or a
        photo.Frame (photo.crop_regions: a batch without a rolled frame is one crop_resize call).  seeds: a noise.Seeds over the pairs (the
        photo's seed, the face's rank as the sub-stream) for every draw of the pass, or None.  teacher = (tau, feather, strengths, warp):
        every crop gets its x_p from its own crop, its reference's crop and their label maps (crop-resized ``src_segs`` / ``ref_segs``,
        else parsed), with the warped term where ``warp`` (_mask_points_warp) is not empty, and the pass starts from it
        (_teacher_start); None: the pass as before"""
        eng = self._require_engine()
        self._check_unipc_masked()
        need_seg = self.fix_background or self.paste_background or teacher is not None
        cs = eng.crop_regions(src_photos, src_regions, size, labels=src_segs)
        cr = eng.crop_regions(ref_photos, ref_regions, size, **({} if ref_segs is None else {'labels': ref_segs}))
        n = len(src_photos)
        if cr.img01.shape[0] != n:
            raise ValueError(f'{n} source photos but {cr.img01.shape[0]} reference photos')
        src, ref = cs.img01, cr.img01
        ctx = self.get_cond_txt_coding(batch if batch is not None else {self.cond_stage_key: ['makeup transfer'] * n})
        cond = {'c_concat': [torch.cat((src, ref), 1)], 'c_crossattn': [ctx]}
        extra = {} if x_T is None else {'x_T': x_T.to(self.device)}
        if seeds is not None:
            extra['seeds'] = seeds
        seg_batch = {self.seg_key: cs.labels if (src_segs is not None or not need_seg) else self.parse_images(src)}
        if self.fix_background:
            x0, mask = self.background_latents(seg_batch, src, seeds=seeds)
            extra.update(x0=x0, mask=mask)
        scale = float(self.unconditional_guidance_scale)
        if scale > 1.0:           # log_results' guided pass: the unconditional branch keeps the SAME hint
            extra.update(unconditional_guidance_scale=scale,
                         unconditional_conditioning={'c_concat': cond['c_concat'], 'c_crossattn': [self.get_unconditional_conditioning(n)]})
            if phi != 0.0:
                extra['guidance_rescale'] = phi
        sample_log = self.sample_log
        if teacher is not None:
            from .. import teacher as _teacher
            tau, t_feather, t_strengths, t_warp = teacher
            x_p = _teacher.pseudo_ground_truth(src, ref, seg_batch[self.seg_key], cr.labels if ref_segs is not None else self.parse_images(ref),
                                               strengths=t_strengths, feather=t_feather, **t_warp)[0]
            sample_log = self._teacher_start(self.get_z(x_p * 2.0 - 1.0, seeds=seeds), seeds, tau)
        lat, _ = sample_log(cond=cond, batch_size=n, ddim=True, ddim_steps=self.ddim_steps, eta=self.ddim_eta, **extra)
        img = self.decode_first_stage(lat)
        if self.paste_background:
            img, _ = self.paste_source(seg_batch, img, src * 2.0 - 1.0)
        return img, src

    @torch.no_grad()
    def transfer_photos(self, src_photos, ref_photos, src_boxes=None, ref_boxes=None, src_segs=None, feather: int = 8,
                        x_T: Optional[torch.Tensor] = None, size: int = 256, batch: Optional[dict] = None,
                        guidance_rescale: Optional[float] = None, max_faces: Optional[int] = None, face_batch: int = 8,
                        return_faces: bool = False, own_pixels: bool = False, own_feather: int = 2, align: bool = False,
                        min_roll: float = 5.0, guided_paste=None, seeds=None, teacher_start: Optional[float] = None, teacher_feather: int = 2,
                        teacher_strengths=None, ref_segs=None):
        """Makeup transfer on photographs at their own resolution: ``src_photos`` / ``ref_photos`` are uint8 [H,W,3] tensors of any
        size (lists; the photos of a call may differ in size) with a face box (x0, y0, w, h) each.  Both boxes are crop-resized to
        ``size`` on the device (photo.crop_resize: Pillow's antialiased bilinear bytes / 255, what PairFolderDataset gives for that
        crop), ONE sampling pass runs as in transfer_regions -- the ``sampler`` attribute's solver for ddim_steps from x_T, guided when
        unconditional_guidance_scale > 1, with the fix_background / paste_background settings on the crop-resized ``src_segs`` (label
        maps at photo resolution) -- the latent is decoded and pasted into CLONES of the source photos with their fine detail kept
        (photo.paste_photos, ``feather`` photo pixels at the box sides).  ``batch`` carries the text fields get_input reads (txt_emb /
        txt_tokens / txt); without it the prompt is 'makeup transfer'.  ``guidance_rescale`` (default: the model's setting): the phi
        of the guided pass.  With a face parser attached, ``src_segs`` may be None (the crop-resized source is parsed instead) and so
        may ``src_boxes`` / ``ref_boxes`` (face_parser.find_boxes: single-face localisation on the squashed photo).  Returns the uint8
        [H,W,3] device tensors.

        GROUP PHOTOS, ``max_faces`` = K >= 1 (None: everything above, unchanged; this rule is this build's).  Every source photo is
        fanned out into up to K crops, one per face: ``src_boxes`` None takes face_parser.find_faces(max_faces=K) (connected components
        of the face classes, largest first); else entry i of ``src_boxes`` is a LIST of 0..K boxes of photo i and no parser is needed.
        ``ref_boxes`` None takes the LARGEST face of every reference (find_faces(max_faces=1); a reference without one raises
        ValueError naming its index); else one box per reference.  Every face of source photo i uses reference i, label map
        src_segs[i] and the text of entry i of ``batch``.  The work items are the N = sum of faces crops in photo-major, rank-minor
        order; ``x_T`` is [N,4,h,w] in that order.  Sampling, decode and paste_source run in chunks of at most ``face_batch`` items, the
        ragged last chunk as a call of its own, each chunk exactly the single pass above for a batch of that size.  The results are
        pasted into ONE clone per source photo rank by rank (one paste_photos call for rank 0 of every photo that has one, then rank 1,
        ...), so a photo never appears twice in a launch and stream order fixes what overlapping boxes give: the larger face is pasted
        first, and a smaller face that overlaps it adds ITS difference (against its crop of the ORIGINAL photo) on top of pixels the
        first paste may already have changed.  A crop may show part of a neighbouring face, which the model is free to change: by
        default the paste is not restricted to the face's own component.  A photo without a face comes back as an unchanged clone;
        N = 0 samples nothing.  ``return_faces``: (photos, the list of box lists) instead of the photos.

        ``own_pixels`` (with max_faces, faces from the attached parser only: src_boxes None, else ValueError): every face's paste
        stays on its own pixels.  find_faces(return_owner=True) also gives the owner map, the nearest component of every pixel of
        the squashed map (every component of at least min_area pixels is a seed, also those beyond K); the paste of rank k of photo
        i is weighted by components.owner_weights (the fraction of the (2 own_feather + 1)^2 parse-pixel window that rank k owns,
        upsampled to the photo by mkd_paste_photo_weighted), so what a crop shows of a neighbour is not written, a face beyond K
        keeps its bytes, and the weights of neighbouring faces sum to one across their border.

        ``align`` (with max_faces; off: everything above, untouched; this rule is this build's): TILTED FACES.  Source and reference
        faces are cropped along oriented squares (photo.Frame) so that the model sees every face upright, and the results are pasted
        back along them (photo.crop_frames / paste_frames; with own_pixels the weight plane goes into paste_frames).  The faces come
        from the attached parser -- face_parser.find_faces(oriented=True, min_roll=``min_roll``): the roll is measured on the device
        from the two eye classes, and a face rolled by less than min_roll degrees keeps exactly its axis-aligned box -- or from caller
        boxes that carry the roll as a fifth entry, (x0, y0, w, h, angle_deg) with w == h (a 4-tuple, or angle 0, is an upright box;
        a photo.Frame instance is taken as it is).
        An upright face takes the crop_resize / paste_photos calls above, so a batch without a rolled face is the path above call for
        call.  ``return_faces`` then gives boxes for caller boxes that are upright and photo.Frame's for everything else.

        ``guided_paste`` (a photo.GuidedPaste; None: everything above, call for call): EVERY paste of the call -- single face, max_faces,
        own_pixels, align -- upsamples the makeup difference under the photo's own luminance edges instead of bilinearly
        (mkd_paste_photo_guided / mkd_paste_frame_guided), so lipstick stops at the lip line of the PHOTO and not a model pixel past it.

        ``seeds`` (default: the model's ``seed``; None: the torch draws, call for call): one seed per SOURCE PHOTO (an int s: s, s + 1,
        ...).  The face of rank k of photo i draws everything -- start latent, eta rows, blend rows, the encoder's posterior -- from
        noise.normal with (seed_i, sub = k), so a face's noise does not depend on face_batch, on max_faces or on the other photos of
        the call.  Without max_faces every face is rank 0.

        ``teacher_start`` = tau in (0, 1] (None: everything above, call for call): TEACHER-STARTED sampling.  Every face crop gets the
        histogram-matching teacher's x_p (teacher.pseudo_ground_truth with ``teacher_feather`` and ``teacher_strengths``, a dict of
        numbers for lip / eye / skin) from its own crop, its reference's crop and their label maps -- ``src_segs`` and ``ref_segs``
        (label maps of the references at photo resolution) crop-resized, or the crops parsed by the attached parser -- and the pass
        runs the last k = teacher.start_steps(tau, ddim_steps) steps from stochastic_encode(get_z(2 x_p - 1), k - 1).  It needs the
        first-stage encoder; x_T, fix_background, an engaged guidance_rescale and ddim_eta != 0 are refused (ValueError).  A model with
        teacher_warp is refused too (crops carry no landmarks) unless it has teacher_points='masks': then every crop's x_p carries the
        warped term, its control points taken from the crop's own region masks (teacher.region_points) and solved on the device."""
        from .. import photo
        from ..components import owner_weights
        from ..face_parser import find_boxes, find_faces
        self._check_unipc_masked()
        phi = float(self.guidance_rescale if guidance_rescale is None else guidance_rescale)
        if not 0.0 <= phi <= 1.0:
            raise ValueError(f'guidance_rescale must lie in [0, 1], got {phi}')
        if guided_paste is not None and not isinstance(guided_paste, photo.GuidedPaste):
            raise ValueError(f'guided_paste must be a photo.GuidedPaste or None, got {guided_paste!r}')
        teach = None
        if teacher_start is not None:
            if self.teacher_warp is not None and self.teacher_points is None:
                raise ValueError('transfer_photos: teacher_start is not combined with teacher_warp (crops carry no landmarks: the warped term '
                                 'of the teacher image needs them in crop pixels)')
            from .. import teacher as _teacher
            _teacher.start_steps(teacher_start, 1)
            _teacher.check_feather(teacher_feather)
            _teacher.strength_rows(teacher_strengths, 1)
            if self.face_parser is None and (src_segs is None or ref_segs is None):
                raise ValueError('transfer_photos: teacher_start needs the label maps of both faces: src_segs and ref_segs, or an attached face parser')
            self._check_teacher_start(x_T, phi)
            teach = (float(teacher_start), int(teacher_feather), teacher_strengths, self._mask_points_warp())
        elif ref_segs is not None or teacher_strengths is not None or teacher_feather != 2:
            raise ValueError('ref_segs / teacher_feather / teacher_strengths only apply with teacher_start')
        # One body for both forms, on regions (boxes or photo.Frame's): the call without max_faces is one face per photo and one chunk
        # of all photos.  Every check comes before the engine is required.
        many = max_faces is not None
        if many:
            K, fb = int(max_faces), int(face_batch)
            if align and not float(min_roll) >= 0.0:
                raise ValueError(f'min_roll must be >= 0 degrees, got {min_roll!r}')
            if own_pixels and (src_boxes is not None or self.face_parser is None):
                raise ValueError('own_pixels needs the faces from the attached face parser (src_boxes None): a box has no component to own pixels')
            if own_pixels and (int(own_feather) != own_feather or not 0 <= int(own_feather) <= 16):
                raise ValueError(f'own_feather must be an integer 0..16 parse pixels, got {own_feather!r}')
            if K != max_faces or not 1 <= K <= 64:
                raise ValueError(f'max_faces must be an integer 1..64, got {max_faces!r}')
            if fb != face_batch or fb < 1:
                raise ValueError(f'face_batch must be an integer >= 1, got {face_batch!r}')
        elif own_pixels:
            raise ValueError('own_pixels only applies with max_faces')
        elif align:
            raise ValueError('align only applies with max_faces')
        elif return_faces or face_batch != 8:
            raise ValueError('return_faces / face_batch only apply with max_faces')
        src_photos, ref_photos = list(src_photos), list(ref_photos)
        n = len(src_photos)
        if len(ref_photos) != n:
            raise ValueError(f'{n} source photos but {len(ref_photos)} reference photos')
        sd = self._seeds(seeds, n) if n else None
        if sd is not None and sd.subs is not None:
            raise ValueError('transfer_photos: seeds are per source photo; the sub-stream is the rank of the face and cannot be given')
        if (src_boxes is None or ref_boxes is None) and self.face_parser is None:
            raise ValueError('transfer_photos: src_boxes and ref_boxes are needed (only an attached face parser can find the faces)')

        def region(b):          # (x0, y0, w, h[, angle]) or a Frame -> the box itself when it is upright, else its Frame
            if isinstance(b, photo.Frame):
                return b
            if len(b) == 4 or float(b[4]) == 0.0:
                return tuple(int(v) for v in b[:4])
            return photo.frame_from_box(b[:4], float(b[4]))

        def work_items(faces):          # photo-major, rank-minor; with max_faces x_T holds one start latent per item
            items = [(i, k) for i, fl in enumerate(faces) for k in range(len(fl))]
            if many and x_T is not None and int(x_T.shape[0]) != len(items):
                raise ValueError(f'x_T must hold one start latent per face, [{len(items)},4,h,w] in photo-major order, got {tuple(x_T.shape)}')
            return items

        # faces: a list of regions per source photo; refs: one region per reference.  None: the parser finds them on the device
        if not many:          # one face per photo, its box as the caller gave it: one 4-entry box per photo (photo.check_box sees to the rest)
            for boxes in (src_boxes, ref_boxes):
                if boxes is not None and len(boxes) != n:
                    raise ValueError(f'{n} photos but {len(boxes)} boxes')
                for b in () if boxes is None else boxes:
                    if len(b) != 4:
                        raise ValueError(f'a box is (x0, y0, w, h), got {b!r}')
            faces = None if src_boxes is None else [[b] for b in src_boxes]
            refs = None if ref_boxes is None else list(ref_boxes)
        else:
            # align: a box may carry the face's roll in degrees as a fifth entry
            is_box = lambda b: isinstance(b, (tuple, list)) and (len(b) == 4 or (align and len(b) == 5)) and not any(isinstance(v, (tuple, list)) for v in b)
            if src_boxes is not None:
                src_boxes = list(src_boxes)
                if len(src_boxes) != n:
                    raise ValueError(f'max_faces: src_boxes must hold one LIST of boxes per source photo ({n}), got {len(src_boxes)} entries')
                for i, bl in enumerate(src_boxes):
                    if not isinstance(bl, (tuple, list)) or not all(is_box(b) for b in bl):
                        raise ValueError(f'max_faces: src_boxes[{i}] must be a list of boxes (x0, y0, w, h), got {bl!r}')
                    if len(bl) > K:
                        raise ValueError(f'max_faces: src_boxes[{i}] holds {len(bl)} boxes, more than max_faces = {K}')
            if ref_boxes is not None:
                ref_boxes = list(ref_boxes)
                if len(ref_boxes) != n or not all(is_box(b) for b in ref_boxes):
                    raise ValueError(f'max_faces: ref_boxes must hold one box (x0, y0, w, h) per reference photo ({n}), got {ref_boxes!r}')
            faces = None if src_boxes is None else [[region(b) for b in bl] for bl in src_boxes]
            refs = None if ref_boxes is None else [region(b) for b in ref_boxes]
        items = None if faces is None else work_items(faces)
        if src_segs is not None and len(src_segs) != n:
            raise ValueError(f'{n} source photos but {len(src_segs)} label maps')
        if ref_segs is not None and len(ref_segs) != n:
            raise ValueError(f'{n} reference photos but {len(ref_segs)} label maps')
        if not self.has_first_stage:
            raise ValueError('transfer_photos pastes decoded images: it needs a first stage (first_stage_config)')
        if (self.fix_background or self.paste_background) and src_segs is None and self.face_parser is None:
            raise KeyError('transfer_photos: fix_background / paste_background need src_segs (label maps at photo resolution)')
        eng = self._require_engine()
        src_photos = [p.to(self.device) for p in src_photos]
        ref_photos = [p.to(self.device) for p in ref_photos]
        look = dict(parse_size=self.parse_size, lut=self.parser_lut)
        if align:          # find_faces returns Frames
            look.update(oriented=True, min_roll=float(min_roll))
        owner = None
        if faces is None:
            if not many:
                faces = [[b] for b in find_boxes(self.face_parser, src_photos, **look)]
            elif own_pixels:
                found, owner = find_faces(self.face_parser, src_photos, max_faces=K, return_owner=True, **look)
                faces = [[region(b) for b in fl] for fl in found]
            else:
                faces = [[region(b) for b in fl] for fl in find_faces(self.face_parser, src_photos, max_faces=K, **look)]
            items = work_items(faces)
        if refs is None:
            if not many:
                refs = find_boxes(self.face_parser, ref_photos, **look)
            else:
                found = find_faces(self.face_parser, ref_photos, max_faces=1, **look)
                for i, fl in enumerate(found):
                    if not fl:
                        raise ValueError(f'transfer_photos: reference photo {i} shows no face')
                refs = [fl[0] for fl in found]
        N = len(items)
        out = [p.clone(memory_format=torch.contiguous_format) for p in src_photos]
        imgs, srcs = [], []
        # without max_faces: ONE chunk of all photos with x_T and batch as they came (an empty call reaches the crop, which refuses it)
        for c0 in range(0, N, fb) if many else (0,):
            chunk = items[c0:c0 + fb] if many else items
            pick = [i for i, _ in chunk]
            text, start = batch, x_T
            if many and batch is not None:          # the text fields get_input reads, one row per face
                idx = torch.tensor(pick)
                text = {k: (v[idx.to(v.device)] if isinstance(v, torch.Tensor) else [v[i] for i in pick])
                        for k, v in batch.items() if k in ('txt_emb', 'txt_tokens', self.cond_stage_key)}
            if many and x_T is not None:
                start = x_T[c0:c0 + len(chunk)]
            face_sd = None
            if sd is not None and chunk:          # the photo's seed, the face's rank
                from ..noise import Seeds
                face_sd = Seeds(tuple(sd.seeds[i] for i in pick), tuple(k for _, k in chunk))
            img, src = self._photo_pass([src_photos[i] for i in pick], [ref_photos[i] for i in pick], [faces[i][k] for i, k in chunk],
                                        [refs[i] for i in pick], None if src_segs is None else [src_segs[i] for i in pick], start, size, text, phi,
                                        **({} if face_sd is None else {'seeds': face_sd}),
                                        **({} if teach is None else {'teacher': teach, 'ref_segs': None if ref_segs is None else [ref_segs[i] for i in pick]}))
            imgs.append(img)
            srcs.append(src)
        if N:
            img, src = (torch.cat(imgs), torch.cat(srcs)) if many else (imgs[0], srcs[0])
            for rank in range(max(len(fl) for fl in faces)):
                sel = [j for j, (_, k) in enumerate(items) if k == rank]
                rows = (img, src)          # without max_faces every item is rank 0: the pass's tensors as they are
                if many:
                    at = torch.tensor(sel, device=img.device)
                    rows = (img[at], src[at])
                # own_pixels: rank k of photo i is row k of its table, the weight that row's share of every neighbourhood
                weights = None if owner is None else owner_weights(owner, [(items[j][0], rank) for j in sel], own_feather)
                eng.paste_regions([out[items[j][0]] for j in sel], [faces[items[j][0]][rank] for j in sel], *rows, feather, weights, guided_paste)
        return (out, faces) if return_faces else out

    def video_session(self, ref_photo, ref_box=None, seed=None, size: int = 256, feather: int = 8, max_faces: int = 4, face_batch: int = 8,
                      align: bool = False, min_roll: float = 5.0, guided_paste=None, temporal=TemporalFilter(), box_smooth: float = 0.5,
                      tracker=None, motion=None, **more):
        """VIDEO CLIPS (this rule is this build's): a session that makes up the frames of ONE clip with the face of ``ref_photo`` (one
        uint8 [H,W,3] tensor, cropped once: ``ref_box``, or the largest face the attached parser finds) without the three kinds of
        flicker transfer_photos has on a sequence.  ``session.push(frames, src_boxes=None, src_segs=None)`` takes the next frames (a
        list of uint8 [H,W,3] tensors; ``src_boxes`` one LIST of boxes per frame, None: the parser finds the faces) and returns the
        made-up frames as clones.  Inside one push: (1) the faces of all pushed frames are found; (2) a video.FaceTracker (``tracker``,
        default FaceTracker()) gives every face a track id and video.smooth_frame (``box_smooth`` = gamma in [0, 0.95]) its crop, frame
        by frame on the host; (3) all (frame, track) items of the push are cropped, sampled and decoded in chunks of ``face_batch``
        through the single pass of transfer_photos, untouched; (4) every item draws with noise.Seeds((seed,), (track id,)) -- ``seed``
        (default: the model's ``seed``; None: the torch draws) is the CLIP's and the track the sub-stream, so one person has one start
        latent, one set of eta rows, blend rows and posterior draws for the whole clip, however the detector orders the faces;
        (5) frame by frame in order, ONE mkd_temporal_diff launch over the frame's faces (``temporal``, a video.TemporalFilter,
        default TemporalFilter(): a motion-aware recursive filter of the makeup difference in the face's own coordinates), then the
        pastes of transfer_photos, rank by rank, largest first.  A track that was not in the previous frame (new, or back after a gap)
        starts its filter and its smoothing over and keeps its noise.  ``temporal=None`` makes no mkd_temporal_diff launch and
        ``box_smooth=0`` leaves the regions as they were found; with both and ``seed=None`` a push is
        transfer_photos(max_faces=...) on its frames, call for call.  ``batch``: ONE row of the text fields get_input reads, the text
        of the clip.  ``session.last`` (a list of video.FrameRecord) tells what the last push did with each frame.  The host
        decisions (tracks, ids, sub-streams, regions) and the noise do not depend on how the clip is split into pushes.  Decoded images
        are equal across BATCH sizes up to rounding only (the GEMM planner picks tiles by shape), so with a seed every chunk is
        sampled at ``face_batch``: a ragged chunk is filled up with repeats of its last item, whose rows are dropped, and the made-up
        frames do not depend on the split either (choose face_batch near faces x frames per push: a one-face push costs a whole
        chunk).  Without a seed the ragged chunk runs as it is, as in transfer_photos.  ``motion`` (a video.MotionSearch, default
        None: off, every call as before): ONE mkd_motion_warp launch in front of every mkd_temporal_diff launch fetches the previous
        state through one integer block-matched vector per block, so the filter holds where something moves inside the crop; it
        needs ``temporal`` (ValueError with temporal=None).  Not combined here, ValueError: ``own_pixels``, per-track references,
        ``teacher_start`` (as a keyword or on the model; video.VideoSession refuses it, so transfer_video does too)."""
        from .. import video
        return video.VideoSession(self, ref_photo, ref_box=ref_box, seed=seed, size=size, feather=feather, max_faces=max_faces,
                                  face_batch=face_batch, align=align, min_roll=min_roll, guided_paste=guided_paste, temporal=temporal,
                                  box_smooth=box_smooth, tracker=tracker, motion=motion, **more)

    def transfer_video(self, frames, ref_photo, frame_batch: int = 8, **session_kwargs):
        """a whole clip: one video_session(ref_photo, **session_kwargs) fed ``frame_batch`` frames at a time (``src_boxes`` /
        ``src_segs``: per frame, over the whole clip) -> the made-up frames"""
        from .. import video
        return video.transfer_video(self, frames, ref_photo, frame_batch, **session_kwargs)

    def test_step(self, batch: dict, batch_idx: int, x_T: Optional[torch.Tensor] = None, seeds=None) -> Dict[str, torch.Tensor]:
        """reference diffusion_makeup.py:332-341.  x_T (not in the reference, which always draws fresh noise): fixed start
        noise for both sampling passes, so that runs can be compared.  seeds: log_results'."""
        images = self.log_results(batch, batch_idx, x_T=x_T, **({} if seeds is None else {'seeds': seeds}))
        for k in images:
            if isinstance(images[k], torch.Tensor):
                images[k] = images[k].detach().cpu()
                if self.clamp and not k.endswith('_latent') and not k.startswith('makeup_hist'):
                    images[k] = torch.clamp(images[k], -1.0, 1.0)
        if self.save_images:
            self.save_local(images, batch_idx)
        return images

    def save_local(self, images: Dict[str, torch.Tensor], batch_idx: int) -> List[str]:
        """One PNG grid per image-valued log entry under saved_dir/model_name (diffusion_makeup.py:344-358; the
        reference's nrow = number of log entries is kept).  Latents (4 channels) are not images and are skipped."""
        from ..imageio import save_grid_png
        root = os.path.join(self.saved_dir, self.model_name)
        # (the scores and the paste weights are not log rows: the grids keep their layout, the PNG names stay the usual ones)
        nrow = len([k for k in images if not k.startswith('makeup_hist') and k != 'mask_pixel'])
        written = []
        for k, v in images.items():
            if not isinstance(v, torch.Tensor) or v.dim() != 4 or v.shape[1] not in (1, 3) or k == 'mask_pixel':
                continue
            written.append(save_grid_png(v, os.path.join(root, '{}_{:04}.png'.format(k, batch_idx)), nrow, self.rescale))
        return written
