"""DPM-Solver++ multistep sampler (host logic): the call surface of UPSTREAM ``ldm.models.diffusion.dpm_solver.DPMSolverSampler``
over the data-prediction multistep solver of Lu et al. 2022 (Algorithm 2; ``multistep_dpm_solver_{second,third}_update`` of the
published ``dpm_solver``), deterministic, eps parameterisation.

It runs on the step grid and tables of ``DDIMSampler.make_schedule(S)``: table entry i goes from ``ddim_alphas[i]`` to
``ddim_alphas_prev[i]`` with the model evaluated at the integer ``ddim_timesteps[i]``, i = S-1 .. 0.  (Upstream's wrapper evaluates
at fractional timesteps of a continuous-time schedule; the engine's timesteps are int64, so that form is not built: DESIGN.md §0.)
Every step is ``x <- c_x x + c_0 m_k + c_1 m_{k-1} + c_2 m_{k-2}`` with m_k = (x - sigma_t e) / alpha_t the x0-prediction of executed
step k and six schedule-only numbers per step (include/mkd.h mkd_dpmpp_table).  Order 1 is algebraically the eta = 0 DDIM step.
This module holds the coefficients; the class is ``sampling.MultistepSampler`` with the 'dpmpp' record (the host update is there too)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .ddim import _check_seeds
from .sampling import SOLVERS, MultistepSampler, start_latent

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


class DPMSolverSampler(MultistepSampler):
    solver = SOLVERS['dpmpp']

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, x_T=None, unconditional_guidance_scale=1., unconditional_conditioning=None,
               order=2, lower_order_final=True, callback=None, mask=None, x0=None, log_every_t=100, guidance_rescale=0.0, seeds=None,
               **kw):
        """intermediates as DDIMSampler's: x_inter / pred_x0 = [x_T, one entry per step with index % log_every_t == 0 or the first
        executed one] (pred_x0: the solver's m_k), from the in-library loop's trace or the step loop alike.  guidance_rescale = phi in
        [0, 1], engaged with guidance and phi > 0.  ``seeds`` (as DDIMSampler.sample's): x_T from noise.normal on
        stream 0 unless given, the masked blend's rows on stream 2 (row = executed step); no torch generator is advanced."""
        return self._sample(S, batch_size, shape, conditioning, x_T, unconditional_guidance_scale, unconditional_conditioning,
                            (order, lower_order_final), callback, mask, x0, log_every_t, guidance_rescale, seeds, kw)

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
        img = start_latent(size, x_T, None if seeds is None else _check_seeds(seeds, len(rows)), self.model.device)
        if tuple(img.shape) != size:
            raise ValueError(f'sample_specs: x_T must be {size}, got {tuple(img.shape)}')
        return fast(img, conditioning, rows, 'dpmpp', unconditional_conditioning, None, 1.0)

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None, order=2,
               lower_order_final=True, callback=None):
        """Reverse loop over ddim_timesteps[:t_start], newest first (the loop MKDDIMSampler.reconstruct runs, on the schedule of the
        last make_schedule): regenerates a latent inverted with DDIMSampler.encode(x0, t_enc=t_start)."""
        return self._decode(x_latent, cond, t_start, unconditional_guidance_scale, unconditional_conditioning, (order, lower_order_final),
                            callback)

    # the loop over the first n entries of the current schedule under its earlier signature (tests drive a prefix of a grid with it)
    def _loop(self, img, cond, n, scale, uc, order, lower_order_final, callback, mask, x0, trace=None, phi=0.0, seeds=None):
        return self._run(img, cond, n, scale, uc, (order, lower_order_final), callback, mask, x0, trace, phi, seeds)
