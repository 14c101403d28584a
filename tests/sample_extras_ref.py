"""Restatement of the sampling loop's extras (test infrastructure only): the log-row rule of UPSTREAM DDIMSampler.ddim_sampling's
intermediates, guidance rescale (Lin et al. 2023, section 3.4, on eps: DESIGN.md section 0) in float64, and the DDIM / DPM-Solver++
loops with both, driven by an ``eps_fn`` like masked_sampling_ref.masked_ddim and dpm_solver_ref.dpm_solver_pp."""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

import dpm_solver_ref as dref
import masked_sampling_ref as mref
from oracle import sampler

Tensor = torch.Tensor


def logged_entries(n_steps: int, log_every_t: int) -> List[int]:
    """table entries i that are logged, in execution order (executed step k runs entry i = n_steps - 1 - k):
    ``i % log_every_t == 0 or i == n_steps - 1``"""
    return [i for i in range(n_steps - 1, -1, -1) if i % log_every_t == 0 or i == n_steps - 1]


def guided_f32(e_c: Tensor, e_u: Tensor, scale: float) -> Tensor:
    """g = fmaf(scale, e_c - e_u, e_u) as the kernels form it: the fp32 difference, then ONE rounding of scale * d + e_u (the product
    of two floats is exact in double; the double sum is rounded to float: a double rounding only within 2^-29 ulp of a tie)"""
    d = (e_c.float() - e_u.float()).double()
    return (float(np.float32(scale)) * d + e_u.float().double()).float()


def rescale_factor64(e_c: Tensor, e_u: Tensor, scale: float, phi: float, g: Optional[Tensor] = None) -> Tensor:
    """k [B] in float64: phi std(e_c[b]) / std(g[b]) + (1 - phi) over each sample's elements, two-pass unbiased std; std(g) == 0: 1.
    g: the guided eps to take the std of (default: the exact float64 combine of the inputs)"""
    B = e_c.shape[0]
    c = e_c.double().reshape(B, -1)
    gg = (e_u.double() + float(scale) * (e_c.double() - e_u.double()) if g is None else g.double()).reshape(B, -1)
    if c.shape[1] < 2:
        return torch.ones(B, dtype=torch.float64)
    s_c, s_g = c.std(dim=1), gg.std(dim=1)
    k = torch.ones(B, dtype=torch.float64)
    nz = s_g > 0
    k[nz] = float(phi) * s_c[nz] / s_g[nz] + (1.0 - float(phi))
    return k


def rescaled_eps(e_c: Tensor, e_u: Tensor, scale: float, phi: float) -> Tensor:
    """the eps a rescaled guided step uses, in the dtype of the inputs"""
    g = e_u + scale * (e_c - e_u)
    k = rescale_factor64(e_c, e_u, scale, phi).to(g.dtype)
    return g * k.view(-1, *([1] * (g.dim() - 1)))


def _eps(eps_fn, img, ts, cond, scale, uc, phi, factors):
    if uc is None or scale == 1.0:
        return eps_fn(img, ts, cond)
    cc = {key: (None if cond[key] is None else [torch.cat([u, v]) for u, v in zip(uc[key], cond[key])]) for key in cond}
    e_u, e_c = eps_fn(torch.cat([img, img]), torch.cat([ts, ts]), cc).chunk(2)
    if phi == 0.0:
        return e_u + scale * (e_c - e_u)
    if factors is not None:
        factors.append(rescale_factor64(e_c, e_u, scale, phi))
    return rescaled_eps(e_c, e_u, scale, phi)


def ddim_loop(eps_fn: Callable, sch: 'sampler.Schedule', x_T: Tensor, cond, scale: float = 1.0, uc=None, phi: float = 0.0,
              log_every_t: int = 100, x0: Optional[Tensor] = None, mask: Optional[Tensor] = None, q_draws=None, eta_draws=None,
              temperature: float = 1.0, factors: Optional[list] = None):
    """UPSTREAM ddim_sampling over sch.ddim_timesteps (make_ddim done by the caller) -> (latent, x_inter rows, pred_x0 rows): the
    rows of the logged steps in execution order, WITHOUT the leading x_T entry of the sampler's lists.  mask / x0 / q_draws: the blend
    before every step; eta_draws[i]: the step's noise or None; factors (a list) collects each step's k [B]."""
    n = len(sch.ddim_timesteps)
    sa, s1 = mref.sqrt_tables(sch.num_timesteps)
    img, xs, x0s = x_T, [], []
    for i, step in enumerate(np.flip(sch.ddim_timesteps)):
        index = n - i - 1
        if mask is not None:
            img = mref.blend(img, x0, mask, float(sa[int(step)]), float(s1[int(step)]), q_draws[i])
        ts = torch.full((x_T.shape[0],), int(step), dtype=torch.long)
        e_t = _eps(eps_fn, img, ts, cond, scale, uc, phi, factors)
        nz = None if eta_draws is None else eta_draws[i]
        img, p0 = sampler.denoising_step(lambda *_: e_t, sch, img, None, ts, index, temperature=temperature, noise=nz)
        if index % log_every_t == 0 or index == n - 1:
            xs.append(img); x0s.append(p0)
    return img, xs, x0s


def dpm_loop(eps_fn: Callable, timesteps, alphas, alphas_prev, x_T: Tensor, cond=None, order: int = 2, lower_order_final: bool = True,
             scale: float = 1.0, uc=None, phi: float = 0.0, log_every_t: int = 100, blend: Optional[Callable] = None,
             factors: Optional[list] = None):
    """dpm_solver_ref.dpm_solver_pp with the trace and the rescale -> (latent, x_inter rows, pred_x0 rows = m_k of the logged steps)"""
    import math
    n = len(timesteps)
    orders = dref.step_orders(n, order, lower_order_final)
    img, hist, lams, xs, x0s = x_T, [], [], [], []
    for k in range(n):
        i = n - 1 - k
        step = int(timesteps[i])
        a_t, a_p = float(alphas[i]), float(alphas_prev[i])
        if blend is not None:
            img = blend(k, step, img)
        ts = torch.full((x_T.shape[0],), step, dtype=torch.long)
        e = _eps(eps_fn, img, ts, cond, scale, uc, phi, factors)
        m0 = (img - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
        img = dref.update(img, m0, hist[-1] if k >= 1 else None, hist[-2] if k >= 2 else None, a_t, a_p,
                          lams[-1] if k >= 1 else 0.0, lams[-2] if k >= 2 else 0.0, orders[k])
        hist.append(m0)
        lams.append(dref.lam(a_t))
        if i % log_every_t == 0 or i == n - 1:
            xs.append(img); x0s.append(m0)
    return img, xs, x0s
