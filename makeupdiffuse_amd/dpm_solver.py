"""DPM-Solver++ multistep sampler (host logic): the call surface of UPSTREAM ``ldm.models.diffusion.dpm_solver.DPMSolverSampler``
over the data-prediction multistep solver of Lu et al. 2022 (Algorithm 2; ``multistep_dpm_solver_{second,third}_update`` of the
published ``dpm_solver``), deterministic, eps parameterisation.

It runs on the step grid and tables of ``DDIMSampler.make_schedule(S)``: table entry i goes from ``ddim_alphas[i]`` to
``ddim_alphas_prev[i]`` with the model evaluated at the integer ``ddim_timesteps[i]``, i = S-1 .. 0.  (Upstream's wrapper evaluates
at fractional timesteps of a continuous-time schedule; the engine's timesteps are int64, so that form is not built: DESIGN.md §0.)
Every step is ``x <- c_x x + c_0 m_k + c_1 m_{k-1} + c_2 m_{k-2}`` with m_k = (x - sigma_t e) / alpha_t the x0-prediction of executed
step k and six schedule-only numbers per step (include/mkd.h mkd_dpmpp_table).  Order 1 is algebraically the eta = 0 DDIM step."""
from __future__ import annotations

import math

import numpy as np
import torch

from .ddim import DDIMSampler, _check_mask, _check_rescale, _check_seeds, rescale_guided_eps

__all__ = ['DPMSolverSampler', 'dpmpp_coefficients']


def dpmpp_coefficients(alphas, alphas_prev, order=2, lower_order_final=True):
    """float64 ``(coef [n, 6], step_order [n])`` of the multistep DPM-Solver++ on a DDIM table: row i = 1/alpha_t, sigma_t, c_x,
    c_0, c_1, c_2 of table entry i (executed step k = n - 1 - i).  The same arithmetic as mkd_dpmpp_table, which stores it as float."""
    n = len(alphas)
    if order not in (1, 2, 3):
        raise ValueError('DPM-Solver++: order must be 1, 2 or 3')
    if n <= 0 or len(alphas_prev) != n:
        raise ValueError('DPM-Solver++: alphas / alphas_prev must be non-empty and equally long')
    coef = np.zeros((n, 6), dtype=np.float64)
    orders = np.zeros(n, dtype=np.int32)
    lam1 = lam2 = 0.0                                    # lambda at the evaluations of executed steps k - 1, k - 2
    for k in range(n):
        i = n - 1 - k
        a_t, a_p = float(alphas[i]), float(alphas_prev[i])
        if not (0.0 < a_t < 1.0 and 0.0 < a_p < 1.0):
            raise ValueError('DPM-Solver++: every alpha must lie in (0, 1)')
        lam_t, lam_p = 0.5 * math.log(a_t / (1.0 - a_t)), 0.5 * math.log(a_p / (1.0 - a_p))
        h = lam_p - lam_t
        if not h > 0.0 or (k > 0 and not lam_t > lam1):
            raise ValueError('DPM-Solver++: lambda must increase along the executed steps')
        p = min(order, k + 1)
        if lower_order_final and n < 10:
            p = min(p, n - k)
        alpha_p, phi1 = math.sqrt(a_p), math.expm1(-h)
        c0, c1, c2 = -alpha_p * phi1, 0.0, 0.0
        if p == 2:
            r0 = (lam_t - lam1) / h
            c0 = -alpha_p * phi1 * (1.0 + 0.5 / r0)
            c1 = alpha_p * phi1 * 0.5 / r0
        elif p == 3:
            r0, r1 = (lam_t - lam1) / h, (lam1 - lam2) / h
            phi2 = phi1 / h + 1.0
            phi3 = phi2 / h - 0.5
            w, q = r0 / (r0 + r1), 1.0 / (r0 + r1)
            g0 = alpha_p * (phi2 * (1.0 + w) - phi3 * q)          # coefficient of D1_0 = (m_k - m_{k-1}) / r0
            g1 = alpha_p * (phi3 * q - phi2 * w)                  # coefficient of D1_1 = (m_{k-1} - m_{k-2}) / r1
            c0 = -alpha_p * phi1 + g0 / r0
            c1 = g1 / r1 - g0 / r0
            c2 = -g1 / r1
        coef[i] = (1.0 / math.sqrt(a_t), math.sqrt(1.0 - a_t), math.sqrt(1.0 - a_p) / math.sqrt(1.0 - a_t), c0, c1, c2)
        orders[i] = p
        lam2, lam1 = lam1, lam_t
    return coef, orders


class DPMSolverSampler:
    # options of upstream samplers that this deterministic solver does not have
    _REJECTED = ('score_corrector', 'corrector_kwargs', 'dynamic_threshold', 'ucg_schedule', 'img_callback', 'quantize_x0')

    def __init__(self, model, **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self._ddim = DDIMSampler(model)          # the step grid, its tables, the guidance batching and the masked blend

    def make_schedule(self, num_steps, verbose=False):
        """The grid of DDIMSampler.make_schedule(num_steps): ddim_timesteps / ddim_alphas / ddim_alphas_prev."""
        self._ddim.make_schedule(ddim_num_steps=num_steps, ddim_eta=0.0, verbose=verbose)
        self.ddim_timesteps = self._ddim.ddim_timesteps
        self.ddim_alphas = self._ddim.ddim_alphas
        self.ddim_alphas_prev = self._ddim.ddim_alphas_prev

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
               order=2, lower_order_final=True, callback=None, mask=None, x0=None, log_every_t=100, guidance_rescale=0.0, seeds=None,
               **kw):
        """intermediates as DDIMSampler's: x_inter / pred_x0 = [x_T, one entry per step with index % log_every_t == 0 or the first
        executed one] (pred_x0: the solver's m_k), from the in-library loop's trace or the step loop alike.  guidance_rescale = phi in
        [0, 1], engaged with guidance and phi > 0.  ``seeds`` (as DDIMSampler.sample's): x_T from noise.normal on
        stream 0 unless given, the masked blend's rows on stream 2 (row = executed step); no torch generator is advanced."""
        if kw.get('eta') not in (None, 0, 0.0):
            raise NotImplementedError('DPMSolverSampler is deterministic: eta is not an option of DPM-Solver++')
        for k in self._REJECTED:
            if kw.get(k) not in (None, False):
                raise NotImplementedError(f'DPMSolverSampler.sample option {k} is not on the MakeupDiffuse path')
        if kw.get('temperature', 1.0) != 1.0 or kw.get('noise_dropout', 0.0) != 0.0:
            raise NotImplementedError('DPMSolverSampler draws no noise: temperature / noise_dropout do not apply')
        if order not in (1, 2, 3):
            raise ValueError('DPMSolverSampler: order must be 1, 2 or 3')
        C, H, W = shape
        size = (batch_size, C, H, W)
        _check_mask(mask, x0, size)
        phi = _check_rescale(guidance_rescale)
        if unconditional_conditioning is None or unconditional_guidance_scale == 1.0:
            phi = 0.0          # no unconditional half: not engaged
        if int(log_every_t) < 1:
            raise ValueError(f'log_every_t must be >= 1, got {log_every_t}')
        if seeds is not None:
            seeds = _check_seeds(seeds, batch_size)
        self.make_schedule(S, verbose=False)
        img = self._start(size, x_T, seeds)
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        img = self._loop(img, conditioning, len(self.ddim_timesteps), unconditional_guidance_scale, unconditional_conditioning, order,
                         lower_order_final, callback, mask, x0, trace=(int(log_every_t), intermediates), phi=phi, seeds=seeds)
        if len(intermediates['x_inter']) == 1:          # (a hook that keeps no trace)
            intermediates['x_inter'].append(img)
        return img, intermediates

    def _start(self, size, x_T, seeds):
        """the start latent: x_T as given, else noise.normal on stream 0 with seeds, else a torch draw"""
        if x_T is not None:
            return x_T
        if seeds is not None:
            from .noise import STREAM_START, normal
            return normal(seeds, size[1:], stream=STREAM_START, device=self.model.device)
        return torch.randn(size, device=self.model.device)

    @torch.no_grad()
    def sample_specs(self, specs, shape, conditioning, x_T=None, unconditional_guidance_scale=None, unconditional_conditioning=None,
                     temperature=1.0, seeds=None):
        """``DDIMSampler.sample_specs`` on this solver: one ``SampleSpec`` (steps, guidance, order, t_start; eta must be 0) per sample
        in one loop of max(steps) evaluations.  Sample b gets the bits of ``sample(S=steps_b, order=order_b,
        unconditional_guidance_scale=guidance_b)``.  ``seeds``: x_T from noise.normal on stream 0 unless given."""
        from .batching import build_rows, guided
        if unconditional_guidance_scale is not None:
            raise ValueError('sample_specs: the guidance scale is per sample (SampleSpec.guidance)')
        if temperature != 1.0:
            raise NotImplementedError('DPMSolverSampler draws no noise: temperature does not apply')
        rows = build_rows(specs, self.model.alphas_cumprod, 'dpmpp', self.ddpm_num_timesteps)
        if guided(rows) and unconditional_conditioning is None:
            raise ValueError('sample_specs: a spec with guidance != 1 needs unconditional_conditioning')
        fast = self._ddim._rows_hook('sample_specs')
        C, H, W = shape
        size = (len(rows), C, H, W)
        img = self._start(size, x_T, None if seeds is None else _check_seeds(seeds, len(rows)))
        if tuple(img.shape) != size:
            raise ValueError(f'sample_specs: x_T must be {size}, got {tuple(img.shape)}')
        return fast(img, conditioning, rows, 'dpmpp', unconditional_conditioning, None, 1.0)

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None, order=2,
               lower_order_final=True, callback=None):
        """Reverse loop over ddim_timesteps[:t_start], newest first (the loop MKDDIMSampler.reconstruct runs, on the schedule of the
        last make_schedule): regenerates a latent inverted with DDIMSampler.encode(x0, t_enc=t_start)."""
        if t_start > len(self.ddim_timesteps):
            raise ValueError(f'DPMSolverSampler.decode: t_start {t_start} > {len(self.ddim_timesteps)} schedule steps')
        if t_start <= 0:
            return x_latent
        return self._loop(x_latent, cond, int(t_start), unconditional_guidance_scale, unconditional_conditioning, order, lower_order_final,
                          callback, None, None)

    # the loop over the first n table entries, newest first
    # trace = (log_every_t, the intermediates dict to append to) or None; phi: the engaged guidance rescale (0: off)
    def _loop(self, img, cond, n, scale, uc, order, lower_order_final, callback, mask, x0, trace=None, phi=0.0, seeds=None):
        timesteps = self.ddim_timesteps[:n]
        a = [float(v) for v in self.ddim_alphas[:n]]
        ap = [float(v) for v in self.ddim_alphas_prev[:n]]
        fast = getattr(self.model, 'sample_loop_dpmpp', None)
        if fast is not None and callback is None:
            # the whole loop runs inside libmkd (mkd_sample_dpmpp); masked: the blend's draws are taken here in loop order, as
            # DDIMSampler does, with the DDPM tables at each entry's timestep
            kw = {}
            if mask is not None:
                sa, s1 = self._ddim._q_tables()
                if seeds is not None:
                    from .noise import STREAM_BLEND, normal
                    q_noise = normal(seeds, tuple(x0.shape)[1:], stream=STREAM_BLEND, rows=n, device=x0.device)
                else:
                    q_noise = torch.stack([torch.randn_like(x0) for _ in range(n)])
                kw = dict(x0=x0, mask=mask, q_sqrt_ac=[float(sa[int(t)]) for t in timesteps],
                          q_sqrt_1m_ac=[float(s1[int(t)]) for t in timesteps], q_noise=q_noise)
            if trace is not None:
                kw['log_every_t'] = trace[0]
            if phi != 0.0:
                kw['guidance_rescale'] = phi
            res = fast(img, cond, timesteps, a, ap, order, lower_order_final, scale, uc, **kw)
            if not isinstance(res, tuple):
                return res
            img, x_rows, x0_rows = res          # (latent, x_inter rows, pred_x0 rows); the latent stays the last x_inter entry
            trace[1]['x_inter'] += [*x_rows[:-1], img]
            trace[1]['pred_x0'] += list(x0_rows)
            return img
        step_fn = getattr(self.model, 'dpmpp_step', None)
        on_device = step_fn is not None and img.is_cuda
        if on_device:
            from .engine import dpmpp_table
            coef, _ = dpmpp_table(a, ap, order, lower_order_final)          # the floats the in-library loop uses
        else:
            coef, _ = dpmpp_coefficients(a, ap, order, lower_order_final)
        hist = [None, None]                                  # m_{k-1}, m_{k-2}
        for k in range(n):
            index = n - 1 - k
            step = int(timesteps[index])
            ts = torch.full((img.shape[0],), step, device=img.device, dtype=torch.long)
            if mask is not None:
                img = self._ddim._q_blend(x0, step, mask, img, seeds=seeds, row=k)
            e_c, e_u = self._ddim._eps(img, cond, ts, scale, uc)
            rescale = e_u is not None and phi != 0.0
            if on_device:
                img, m0 = step_fn(img, e_c, e_u, scale, coef[index], hist[0], hist[1], **({'guidance_rescale': phi} if rescale else {}))
            else:
                # host tensors (plumbing with a stand-in model, e.g. CPU tests): the same formulae in torch
                inv_alpha, sigma, cx, c0, c1, c2 = (float(v) for v in coef[index])
                if rescale:
                    e_t = rescale_guided_eps(e_c, e_u, scale, phi)
                else:
                    e_t = e_c if e_u is None else e_u + scale * (e_c - e_u)
                m0 = (img - sigma * e_t) * inv_alpha
                img = cx * img + c0 * m0
                if c1 != 0.0:
                    img = img + c1 * hist[0]
                if c2 != 0.0:
                    img = img + c2 * hist[1]
            hist = [m0, hist[0]]
            if callback:
                callback(k)
            if trace is not None and (index % trace[0] == 0 or index == n - 1):
                trace[1]['x_inter'].append(img)
                trace[1]['pred_x0'].append(m0)
        return img
