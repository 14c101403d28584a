"""Stock DDIM sampler (host logic): what `from ldm.models.diffusion.ddim import *` gives the reference at
diffmk/cddim.py:2 — DDIMSampler with make_schedule / sample / ddim_sampling / p_sample_ddim, `noise_like`
and `np`.  Only the eps parameterisation and the options the reference exercises are implemented; anything
else raises instead of silently diverging.  The loops (fast path, step loop, trace merge, masked-blend keywords, start latent, host
guided eps) are the driver of ``sampling.py``, shared with the multistep solvers."""
from __future__ import annotations

import numpy as np
import torch

from .sampling import SOLVERS, blend_kwargs, fast_loop, guided_eps, rescale_guided_eps, start_latent, step_loop  # noqa: F401
from .schedule import make_ddim_sampling_parameters, make_ddim_timesteps

__all__ = ['DDIMSampler', 'noise_like', 'np', 'torch']

_DDIM = SOLVERS['ddim']          # the hook names and the host update of this solver


def noise_like(shape, device, repeat=False):
    if repeat:
        return torch.randn((1, *shape[1:]), device=device).repeat(shape[0], *((1,) * (len(shape) - 1)))
    return torch.randn(shape, device=device)


def _check_mask(mask, x0, shape):
    """mask / x0 of masked sampling: x0 [B,C,h,w] (the un-doubled batch), mask [1|B, 1|C, h, w]; a mask needs an x0"""
    if mask is None:
        return
    if x0 is None:
        raise ValueError('DDIMSampler: mask needs x0 (the latent to keep where mask = 1)')
    B, C, H, W = shape
    if tuple(x0.shape) != (B, C, H, W):
        raise ValueError(f'DDIMSampler: x0 must be {(B, C, H, W)}, got {tuple(x0.shape)}')
    if mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, C) or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f'DDIMSampler: mask must be [1 or {B}, 1 or {C}, {H}, {W}], got {tuple(mask.shape)}')


def _check_seeds(seeds, batch, noise_dropout=0.0):
    """seeds= of a sampler call as a noise.Seeds of the batch; dropout draws on the torch generator, so the two do not combine"""
    from .noise import as_seeds
    if noise_dropout > 0.0:
        raise ValueError('seeds: noise_dropout draws on the torch generator and cannot be seeded per sample')
    return as_seeds(seeds, batch)


def _check_rescale(phi) -> float:
    """guidance_rescale (phi of Lin et al. 2023, section 3.4) as a float in [0, 1]"""
    phi = float(phi)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f'guidance_rescale must lie in [0, 1], got {phi}')
    return phi


def _cat_cond(uncond, c):
    """CFG batching, unconditional FIRST (diffmk/cddim.py:18-38)."""
    if isinstance(c, dict):
        assert isinstance(uncond, dict)
        out = {}
        for k in c:
            if isinstance(c[k], list):
                out[k] = [torch.cat([uncond[k][i], c[k][i]]) for i in range(len(c[k]))]
            elif c[k] is None:              # c_concat None (the inversion runs the UNet alone)
                out[k] = None
            else:
                out[k] = torch.cat([uncond[k], c[k]])
        return out
    if isinstance(c, list):
        assert isinstance(uncond, list)
        return [torch.cat([uncond[i], c[i]]) for i in range(len(c))]
    return torch.cat([uncond, c])


class DDIMSampler:
    def __init__(self, model, schedule='linear', **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor):
            attr = attr.detach().clone().to(torch.float32).to(getattr(self.model, 'device', 'cpu'))
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize='uniform', ddim_eta=0.0, verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps)
        ac = self.model.alphas_cumprod
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        acn = ac.detach().cpu().to(torch.float32).numpy()
        self.register_buffer('betas', self.model.betas)
        self.register_buffer('alphas_cumprod', ac)
        self.register_buffer('alphas_cumprod_prev', self.model.alphas_cumprod_prev)
        self.register_buffer('sqrt_alphas_cumprod', torch.tensor(np.sqrt(acn)))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', torch.tensor(np.sqrt(1.0 - acn)))
        self.register_buffer('sqrt_recip_alphas_cumprod', torch.tensor(np.sqrt(1.0 / acn)))
        self.register_buffer('sqrt_recipm1_alphas_cumprod', torch.tensor(np.sqrt(1.0 / acn - 1)))
        sig, a, ap = make_ddim_sampling_parameters(acn, self.ddim_timesteps, ddim_eta)
        self.register_buffer('ddim_sigmas', torch.tensor(np.asarray(sig), dtype=torch.float32))
        self.register_buffer('ddim_alphas', torch.tensor(np.asarray(a), dtype=torch.float32))
        self.ddim_alphas_prev = np.asarray(ap)
        self.register_buffer('ddim_sqrt_one_minus_alphas', torch.tensor(np.sqrt(1.0 - a), dtype=torch.float32))
        acp = self.model.alphas_cumprod_prev.detach().cpu().numpy()
        self.register_buffer('ddim_sigmas_for_original_num_steps',
                             torch.tensor(ddim_eta * np.sqrt((1 - acp) / (1 - acn) * (1 - acn / acp)), dtype=torch.float32))

    # -- full sampling from noise (reached from ControlLDM.sample_log, diffmk/diffusion_makeup.py:393-408) --
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, eta=0.0, temperature=1.0, noise_dropout=0.0,
               x_T=None, log_every_t=100, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               verbose=True, guidance_rescale=0.0, seeds=None, **kwargs):
        """``seeds`` (an int: s, s + 1, ...; one per sample; a noise.Seeds): every draw of the call comes from noise.normal -- x_T on stream
        0 (unless ``x_T`` is given: it is taken as it is), the eta rows on stream 1, the masked blend's rows on stream 2, row = executed
        step -- and no torch generator is advanced.  None: the draws below, as ever."""
        for k in ('score_corrector', 'corrector_kwargs', 'dynamic_threshold', 'ucg_schedule'):
            if kwargs.get(k) is not None:
                raise NotImplementedError(f'DDIMSampler.sample option {k} is not on the MakeupDiffuse path')
        if kwargs.get('quantize_x0', False):
            raise NotImplementedError('quantize_x0')
        C, H, W = shape
        size = (batch_size, C, H, W)
        mask, x0 = kwargs.get('mask'), kwargs.get('x0')
        _check_mask(mask, x0, size)
        _check_rescale(guidance_rescale)
        if seeds is not None:
            seeds = _check_seeds(seeds, batch_size, noise_dropout)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        return self.ddim_sampling(conditioning, size, callback=callback, x_T=x_T, log_every_t=log_every_t, seeds=seeds,
                                  temperature=temperature, noise_dropout=noise_dropout,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, mask=mask, x0=x0,
                                  guidance_rescale=guidance_rescale)

    # -- per-sample requests in one batch (batching.SampleSpec; the in-library per-sample loop, mkd_sample_rows) --
    def _rows_hook(self, what):
        fast = getattr(self.model, 'sample_rows_fast', None)
        if fast is None:
            raise NotImplementedError(f'{what} runs inside libmkd only: the model has no sample_rows_fast hook')
        return fast

    @torch.no_grad()
    def sample_specs(self, specs, shape, conditioning, x_T=None, unconditional_guidance_scale=None, unconditional_conditioning=None,
                     temperature=1.0, seeds=None):
        """One ``SampleSpec`` (steps, eta, guidance, t_start) per sample of the batch, all in ONE loop of max(steps) executed steps:
        every sample starts at once and stops after its own steps.  Sample b gets what ``sample(S=steps_b, eta=eta_b,
        unconditional_guidance_scale=guidance_b)`` gives it, bit for bit, with rows 0 .. n_b - 1 of the noise.  Host draw order: x_T
        (unless given), then for each executed step in order one randn of the full batch shape when some active sample has a non-zero
        sigma in it.  The scales come from the specs (``unconditional_guidance_scale`` must stay None); a guided spec needs
        ``unconditional_conditioning``.  No registered buffer of this sampler is touched.  ``seeds`` (as in ``sample``): x_T on stream 0
        and, where some step draws, rows 0 .. S_max - 1 of stream 1 for every sample from noise.normal; sample b reads rows 0 .. n_b - 1
        of its own streams, which is what the uniform call with b's request and b's seed reads."""
        from .batching import build_rows, draw_noise, guided
        if unconditional_guidance_scale is not None:
            raise ValueError('sample_specs: the guidance scale is per sample (SampleSpec.guidance)')
        rows = build_rows(specs, self.model.alphas_cumprod, 'ddim', self.ddpm_num_timesteps)
        if guided(rows) and unconditional_conditioning is None:
            raise ValueError('sample_specs: a spec with guidance != 1 needs unconditional_conditioning')
        fast = self._rows_hook('sample_specs')
        C, H, W = shape
        size = (len(rows), C, H, W)
        device = self.model.device
        if seeds is not None:
            seeds = _check_seeds(seeds, len(rows))
        img = start_latent(size, x_T, seeds, device)
        if tuple(img.shape) != size:
            raise ValueError(f'sample_specs: x_T must be {size}, got {tuple(img.shape)}')
        if seeds is not None:
            from .batching import draw_plan
            from .noise import STREAM_ETA, normal
            plan = draw_plan(rows)
            noise = normal(seeds, size[1:], stream=STREAM_ETA, rows=len(plan), device=device) if any(plan) else None
        else:
            noise = draw_noise(rows, size, device)
        return fast(img, conditioning, rows, 'ddim', unconditional_conditioning, noise, temperature)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, callback=None, log_every_t=100, temperature=1.0, noise_dropout=0.0,
                      unconditional_guidance_scale=1.0, unconditional_conditioning=None, timesteps=None, mask=None, x0=None,
                      guidance_rescale=0.0, seeds=None):
        """mask / x0 (UPSTREAM): before step i, img = q_sample(x0, ts) * mask + (1 - mask) * img with a fresh randn_like(x0) drawn
        BEFORE the step's eta draw; mask = 1 keeps x0, no blend after the last step.  intermediates: x_inter / pred_x0 =
        [x_T, one entry per step with index % log_every_t == 0 or index == total_steps - 1], from the in-library loop's trace or the
        step loop alike.  guidance_rescale = phi in [0, 1], engaged with guidance and phi > 0.  seeds: as in sample."""
        _check_mask(mask, x0, tuple(shape))
        phi = _check_rescale(guidance_rescale)
        if unconditional_conditioning is None or unconditional_guidance_scale == 1.0:
            phi = 0.0          # no unconditional half: not engaged
        device = self.model.device
        if seeds is not None:
            seeds = _check_seeds(seeds, shape[0], noise_dropout)
        img = start_latent(shape, x_T, seeds, device)
        if timesteps is None:
            timesteps = self.ddim_timesteps
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        total_steps = timesteps.shape[0]
        fast = getattr(self.model, _DDIM.loop_hook, None)
        if fast is not None and callback is None:
            # the whole loop runs inside libmkd (mkd_sample / mkd_sample_eta); no per-step host work.  eta > 0: the draws of the
            # stochastic branch (cddim.py:74-78) are taken here, one per step with sigma_t != 0 in loop order - the generator is
            # consumed exactly as by the step-by-step loop below - and handed over as one [steps, ...] tensor
            # masked: the blend's draws too, each step's BEFORE its eta draw (the step loop's order), with the DDPM tables at the
            # step's timestep
            sig = self.ddim_sigmas[:total_steps]
            kw = {}
            stochastic = float(sig.abs().max()) != 0.0
            q_draws = None
            if seeds is not None:
                # one launch per stream fills every row: row k is executed step k (a row whose sigma is 0 is multiplied by it)
                if stochastic:
                    from .noise import STREAM_ETA, normal
                    kw = dict(sigmas=sig, noise=normal(seeds, tuple(shape)[1:], stream=STREAM_ETA, rows=total_steps, device=device),
                              temperature=temperature)
            elif stochastic or mask is not None:
                draws, q_draws = [], []
                for i in range(total_steps):
                    if mask is not None:
                        q_draws.append(torch.randn_like(x0))
                    if not stochastic:
                        continue
                    if float(sig[total_steps - i - 1]) != 0.0:
                        nz = noise_like(tuple(shape), device, False)
                        if noise_dropout > 0.0:
                            nz = torch.nn.functional.dropout(nz, p=noise_dropout)
                    else:
                        nz = torch.zeros(tuple(shape), device=device)
                    draws.append(nz)
                if stochastic:
                    kw = dict(sigmas=sig, noise=torch.stack(draws), temperature=temperature)
            if mask is not None:
                kw.update(blend_kwargs(self._q_tables(), x0, mask, timesteps, seeds, q_draws))
            img = fast_loop(fast, img, cond, (timesteps, self.ddim_alphas[:total_steps], self.ddim_alphas_prev[:total_steps],
                                              self.ddim_sqrt_one_minus_alphas[:total_steps]), unconditional_guidance_scale,
                            unconditional_conditioning, kw, (log_every_t, intermediates), phi)
            if len(intermediates['x_inter']) == 1:          # a hook that keeps no trace
                intermediates['x_inter'].append(img)
            return img, intermediates

        def step(img, ts, index, i):
            return self.p_sample_ddim(img, cond, ts, index=index, temperature=temperature, noise_dropout=noise_dropout, seeds=seeds, row=i,
                                      unconditional_guidance_scale=unconditional_guidance_scale,
                                      unconditional_conditioning=unconditional_conditioning, guidance_rescale=phi)

        blend = None if mask is None else (lambda t, img, i: self._q_blend(x0, t, mask, img, seeds=seeds, row=i))
        return step_loop(img, timesteps, step, callback, blend, (log_every_t, intermediates)), intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1.0, unconditional_conditioning=None, dynamic_threshold=None,
                      guidance_rescale=0.0, seeds=None, row=0):
        """seeds / row: the step's eta noise is noise.normal(seeds, stream 1, row) instead of a torch draw (row = the executed step)"""
        return self._step(x, c, t, index, repeat_noise, use_original_steps, quantize_denoised, temperature, noise_dropout,
                          score_corrector, corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning,
                          dynamic_threshold, _check_rescale(guidance_rescale), seeds, row)

    # One DDIM step; shared by p_sample_ddim and MKDDIMSampler.denoising_step (same arithmetic, SURVEY.md finding 6).
    def _step(self, x, c, t, index, repeat_noise, use_original_steps, quantize_denoised, temperature, noise_dropout,
              score_corrector, corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning,
              dynamic_threshold, guidance_rescale=0.0, seeds=None, row=0):
        b, device = x.shape[0], x.device
        if getattr(self.model, 'parameterization', 'eps') != 'eps':
            raise NotImplementedError("only parameterization 'eps' (yaml :50) is supported")
        if score_corrector is not None:
            raise NotImplementedError('score_corrector is unused by the reference path')
        if quantize_denoised:
            raise NotImplementedError('quantize_denoised needs first_stage_model.quantize (VAE: SURVEY §8f)')
        if dynamic_threshold is not None:
            raise NotImplementedError()
        e_c, e_u = self._eps(x, c, t, unconditional_guidance_scale, unconditional_conditioning)
        alphas = self.model.alphas_cumprod if use_original_steps else self.ddim_alphas
        alphas_prev = self.model.alphas_cumprod_prev if use_original_steps else self.ddim_alphas_prev
        s1m = self.model.sqrt_one_minus_alphas_cumprod if use_original_steps else self.ddim_sqrt_one_minus_alphas
        sigmas = self.ddim_sigmas_for_original_num_steps if use_original_steps else self.ddim_sigmas
        a_t, a_prev, sigma_t, s1m_t = float(alphas[index]), float(alphas_prev[index]), float(sigmas[index]), float(s1m[index])
        noise = None
        if sigma_t != 0.0 and seeds is not None:
            from .noise import STREAM_ETA, normal
            if repeat_noise:
                raise ValueError('seeds: repeat_noise shares one draw across the batch and cannot be seeded per sample')
            noise = normal(_check_seeds(seeds, b, noise_dropout), tuple(x.shape)[1:], stream=STREAM_ETA, row0=int(row), device=device)
        elif sigma_t != 0.0:
            noise = noise_like(x.shape, device, repeat_noise)
            if noise_dropout > 0.0:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        return self._update(x, e_c, e_u, unconditional_guidance_scale, a_t, a_prev, sigma_t, s1m_t, noise, temperature,
                            guidance_rescale)

    # (e_c, e_u) of one step: CFG batches [uncond; cond] through ONE apply_model; e_u None without guidance
    def _eps(self, x, c, t, unconditional_guidance_scale, unconditional_conditioning):
        cfg_on = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.0)
        if not cfg_on:
            return self.model.apply_model(x, t, c), None
        x_in = torch.cat([x] * 2)
        t_in = torch.cat([t] * 2)
        binder = getattr(self.model, 'cfg_conditioning', None)
        c_in = binder(unconditional_conditioning, c) if binder is not None else _cat_cond(unconditional_conditioning, c)
        e_u, e_c = self.model.apply_model(x_in, t_in, c_in).chunk(2)
        return e_c, e_u

    # the eta-DDIM update x_prev(x, eps) with the coefficients of one step: on the device through the model's hook
    def _update(self, x, e_c, e_u, unconditional_guidance_scale, a_t, a_prev, sigma_t, s1m_t, noise, temperature,
                guidance_rescale=0.0):
        rescale = e_u is not None and guidance_rescale != 0.0
        step_fn = getattr(self.model, _DDIM.step, None)
        if step_fn is not None and x.is_cuda:
            kw = {'guidance_rescale': guidance_rescale} if rescale else {}
            return step_fn(x, e_c, e_u, unconditional_guidance_scale, a_t, a_prev, sigma_t, s1m_t, noise, temperature, **kw)
        # host tensors (plumbing with a stand-in model, e.g. CPU tests): same formulae in torch
        e_t = guided_eps(e_c, e_u, unconditional_guidance_scale, guidance_rescale)
        return _DDIM.host_update(x, e_t, (a_t, a_prev, sigma_t, s1m_t), noise, temperature)

    # -- masked sampling / q_sample (UPSTREAM LatentDiffusion.q_sample as ddim_sampling uses it, DDIMSampler.stochastic_encode) --
    def _q_tables(self):
        return self.model.sqrt_alphas_cumprod, self.model.sqrt_one_minus_alphas_cumprod

    def _q_blend(self, x0, step, mask, img, seeds=None, row=0):
        """img = q_sample(x0, step) * mask + (1 - mask) * img with a fresh randn_like(x0) (seeds: noise.normal on stream 2 at ``row``, the
        executed step); on the device through the model's hook"""
        sa, s1 = self._q_tables()
        a, b = float(sa[step]), float(s1[step])
        if seeds is not None:
            from .noise import STREAM_BLEND, normal
            noise = normal(_check_seeds(seeds, x0.shape[0]), tuple(x0.shape)[1:], stream=STREAM_BLEND, row0=int(row), device=x0.device)
        else:
            noise = torch.randn_like(x0)
        return self._q_sample_blend(x0, noise, a, b, mask, img)

    def _q_sample_blend(self, x0, noise, a, b, mask=None, img=None):
        hook = getattr(self.model, 'q_sample_blend', None)
        if hook is not None and x0.is_cuda:
            return hook(x0, noise, a, b, mask, img)
        # host tensors (a stand-in model, e.g. CPU tests): the same formula in torch
        q = a * x0 + b * noise
        return q if mask is None else q * mask + (1.0 - mask) * img

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None, seeds=None):
        """UPSTREAM DDIMSampler.stochastic_encode: sqrt(ddim_alphas)[t] x0 + ddim_sqrt_one_minus_alphas[t] noise (the full DDPM tables
        with use_original_steps); t [B] indexes the table.  With decode(x, cond, t_start) it gives img2img.  ``seeds`` (without ``noise``): the
        noise is noise.normal on stream 2, row 0, and no torch generator is advanced; ``noise`` given: taken as it is."""
        if use_original_steps:
            sa, s1 = self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod
        else:
            sa, s1 = torch.sqrt(self.ddim_alphas), self.ddim_sqrt_one_minus_alphas
        if noise is None and seeds is not None:
            from .noise import STREAM_BLEND, normal
            noise = normal(_check_seeds(seeds, x0.shape[0]), tuple(x0.shape)[1:], stream=STREAM_BLEND, device=x0.device)
        elif noise is None:
            noise = torch.randn_like(x0)
        t = torch.as_tensor(t).reshape(-1).cpu().long()
        if t.numel() == 1:
            t = t.expand(x0.shape[0])
        if t.numel() != x0.shape[0]:
            raise ValueError(f'stochastic_encode: t has {t.numel()} entries for a batch of {x0.shape[0]}')
        if bool((t == t[0]).all()):
            return self._q_sample_blend(x0, noise, float(sa[int(t[0])]), float(s1[int(t[0])]))
        return torch.cat([self._q_sample_blend(x0[i:i + 1], noise[i:i + 1], float(sa[int(t[i])]), float(s1[int(t[i])]))
                          for i in range(x0.shape[0])])

    # -- DDIM inversion (UPSTREAM DDIMSampler.encode; reference pre_dataset.py InvRec) and its reverse loop --
    @torch.no_grad()
    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, callback=None):
        """Deterministic DDIM inversion x0 -> x_{t_enc}: for i < t_enc, with a_next = alphas[i], a = alphas_prev[i],
        x <- sqrt(a_next / a) x + sqrt(a_next) (sqrt(1 / a_next - 1) - sqrt(1 / a - 1)) eps(x, ddim_timesteps[i]).
        That is the eta = 0 DDIM update with a_t := a and a_prev := a_next, executed in the opposite order.  The in-library
        loop (model.sample_loop_fast / mkd_sample) runs index n-1 .. 0, so it is handed MIRRORED tables: entry j is inversion
        step t_enc - 1 - j, with alphas = ddim_alphas_prev, alphas_prev = ddim_alphas, sqrt_one_minus = sqrt(1 - ddim_alphas_prev).
        callback / return_intermediates / use_original_steps take the eager step loop.  The model is evaluated at
        ddim_timesteps[i], the timestep whose coefficients step i uses.  Returns (x_next, {'x_encoded',
        'intermediate_steps'[, 'intermediates']})."""
        n_ref = self.ddpm_num_timesteps if use_original_steps else self.ddim_timesteps.shape[0]
        if t_enc > n_ref:
            raise ValueError(f'DDIMSampler.encode: t_enc {t_enc} > {n_ref} reference steps')
        num_steps = int(t_enc)
        if use_original_steps:
            alphas_next = self.model.alphas_cumprod[:num_steps]
            alphas = self.model.alphas_cumprod_prev[:num_steps]
            timesteps = np.arange(num_steps)
        else:
            alphas_next = self.ddim_alphas[:num_steps]
            alphas = torch.tensor(np.asarray(self.ddim_alphas_prev[:num_steps]), dtype=torch.float32)
            timesteps = self.ddim_timesteps[:num_steps]
        fast = getattr(self.model, 'sample_loop_fast', None)
        if fast is not None and callback is None and not return_intermediates and not use_original_steps and num_steps > 0:
            a = [float(v) for v in alphas][::-1]
            a_next = [float(v) for v in alphas_next][::-1]
            x_next = fast(x0, c, [int(v) for v in timesteps][::-1], a, a_next, [float(np.sqrt(1.0 - np.float32(v))) for v in a],
                          unconditional_guidance_scale, unconditional_conditioning)
            return x_next, {'x_encoded': x_next, 'intermediate_steps': []}
        intermediates, inter_steps = [], []

        def step(x, t, i, _):
            e_c, e_u = self._eps(x, c, t, unconditional_guidance_scale, unconditional_conditioning)
            a_t, a_n = float(alphas[i]), float(alphas_next[i])
            x, _ = self._update(x, e_c, e_u, unconditional_guidance_scale, a_t, a_n, 0.0, float(np.sqrt(1.0 - np.float32(a_t))), None, 1.0)
            if return_intermediates and (i % (num_steps // return_intermediates) == 0 or i >= num_steps - 2):
                intermediates.append(x)
                inter_steps.append(i)
            return x, None

        x_next = step_loop(x0, timesteps, step, callback, forward=True)
        out = {'x_encoded': x_next, 'intermediate_steps': inter_steps}
        if return_intermediates:
            out['intermediates'] = intermediates
        return x_next, out

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None):
        """Reverse loop over ddim_timesteps[:t_start], newest first (UPSTREAM DDIMSampler.decode; the loop
        MKDDIMSampler.reconstruct runs): inverts encode(x0, t_enc=t_start) for an eps that does not depend on x.
        ``t_start`` as a sequence / tensor of length B: sample b runs entries t_start_b - 1 .. 0 of the current schedule in one
        per-sample loop (the edit strength per sample after an inversion) and gets the bits of the scalar call with t_start_b; it
        needs the in-library loop (eta = 0, no callback, no use_original_steps).  A scalar takes the path below unchanged."""
        if isinstance(t_start, (list, tuple, np.ndarray)) or (isinstance(t_start, torch.Tensor) and t_start.dim() > 0):
            from .batching import start_rows
            if use_original_steps or callback is not None:
                raise NotImplementedError('a per-sample t_start runs inside libmkd: no use_original_steps, no callback')
            cfg_on = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.0)
            rows = start_rows(t_start, self.ddim_timesteps, self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sqrt_one_minus_alphas,
                              cfg_scale=float(unconditional_guidance_scale) if cfg_on else 1.0)
            if len(rows) != x_latent.shape[0]:
                raise ValueError(f't_start has {len(rows)} entries for a batch of {x_latent.shape[0]}')
            if float(self.ddim_sigmas[:max(r.n for r in rows)].abs().max()) != 0.0:
                raise NotImplementedError('a per-sample t_start is deterministic: make_schedule with ddim_eta = 0')
            return self._rows_hook('a per-sample t_start')(x_latent, cond, rows, 'ddim', unconditional_conditioning if cfg_on else None,
                                                           None, 1.0)
        timesteps = np.arange(self.ddpm_num_timesteps) if use_original_steps else self.ddim_timesteps
        timesteps = timesteps[:t_start]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        fast = getattr(self.model, 'sample_loop_fast', None)
        if (fast is not None and callback is None and not use_original_steps and total_steps > 0
                and float(self.ddim_sigmas[:total_steps].abs().max()) == 0.0):
            return fast(x_latent, cond, timesteps, self.ddim_alphas[:total_steps], self.ddim_alphas_prev[:total_steps],
                        self.ddim_sqrt_one_minus_alphas[:total_steps], unconditional_guidance_scale,
                        unconditional_conditioning)
        return step_loop(x_latent, timesteps, lambda x, ts, index, i: self._step(
            x, cond, ts, index, False, use_original_steps, False, 1.0, 0.0, None, None, unconditional_guidance_scale,
            unconditional_conditioning, None), callback)
