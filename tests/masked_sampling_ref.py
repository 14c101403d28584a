"""CPU restatement of masked DDIM sampling (test infrastructure only): UPSTREAM ldm DDIMSampler.ddim_sampling with mask / x0,
LatentDiffusion.q_sample, DDIMSampler.stochastic_encode, and the label map -> latent mask of background-preserving transfer
(the reference's Fixbackground classes, averaged over each f x f block like F.interpolate(mode='area'))."""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional

import numpy as np
import torch

from oracle import sampler

Tensor = torch.Tensor


def sqrt_tables(num_timesteps: int = 1000, linear_start: float = 0.00085, linear_end: float = 0.0120):
    """model.sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod (fp32, from the float64 cumulative product, as upstream registers them)"""
    ac = sampler.Schedule(num_timesteps, linear_start, linear_end).alphas_cumprod64
    return torch.tensor(np.sqrt(ac), dtype=torch.float32), torch.tensor(np.sqrt(1.0 - ac), dtype=torch.float32)


def q_sample(x0: Tensor, sqrt_ac: float, sqrt_1m_ac: float, noise: Tensor) -> Tensor:
    return sqrt_ac * x0 + sqrt_1m_ac * noise


def blend(img: Tensor, x0: Tensor, mask: Tensor, sqrt_ac: float, sqrt_1m_ac: float, noise: Tensor) -> Tensor:
    """img = q_sample(x0, ts) * mask + (1 - mask) * img"""
    return q_sample(x0, sqrt_ac, sqrt_1m_ac, noise) * mask + (1.0 - mask) * img


def masked_ddim(eps_fn: Callable, sch: 'sampler.Schedule', x_T: Tensor, cond, x0: Tensor, mask: Tensor, q_draws: List[Tensor],
                eta_draws: Optional[List[Optional[Tensor]]] = None, scale: float = 1.0, uc=None, temperature: float = 1.0,
                sqrt_ac: Optional[Tensor] = None, sqrt_1m_ac: Optional[Tensor] = None) -> Tensor:
    """The upstream loop written out over sch.ddim_timesteps (sch.make_ddim(steps, eta) done by the caller): before step i the blend
    with q_draws[i], then the eta-DDIM step with eta_draws[i] (None: no noise).  No blend after the last step."""
    if sqrt_ac is None:
        sqrt_ac, sqrt_1m_ac = sqrt_tables(sch.num_timesteps)
    n = len(sch.ddim_timesteps)
    img = x_T
    for i, step in enumerate(np.flip(sch.ddim_timesteps)):
        index = n - i - 1
        img = blend(img, x0, mask, float(sqrt_ac[int(step)]), float(sqrt_1m_ac[int(step)]), q_draws[i])
        ts = torch.full((x_T.shape[0],), int(step), dtype=torch.long)
        if uc is None or scale == 1.0:
            e_t = eps_fn(img, ts, cond)
        else:                                                # [uncond; cond] through one evaluation (c_concat None passes through)
            cc = {k: (None if cond[k] is None else [torch.cat([u, v]) for u, v in zip(uc[k], cond[k])]) for k in cond}
            e_u, e_c = eps_fn(torch.cat([img, img]), torch.cat([ts, ts]), cc).chunk(2)
            e_t = e_u + scale * (e_c - e_u)
        nz = None if eta_draws is None else eta_draws[i]
        img, _ = sampler.denoising_step(lambda *_: e_t, sch, img, None, ts, index, temperature=temperature, noise=nz)
    return img


def latent_mask(labels: np.ndarray, classes: Iterable[int] = (0, 11, 12), factor: int = 8, threshold: float = 0.5) -> np.ndarray:
    """labels [B, H, W] integer -> [B, 1, H/f, W/f] float32: the fraction of each f x f block whose label is in `classes`
    (count / f^2 in fp32); threshold > 0: 1.0 where that fraction >= threshold, else 0.0"""
    lab = np.asarray(labels)
    B, H, W = lab.shape
    assert H % factor == 0 and W % factor == 0
    hit = np.isin(lab, np.asarray(list(classes))).astype(np.int64)
    cnt = hit.reshape(B, H // factor, factor, W // factor, factor).sum(axis=(2, 4))
    frac = cnt.astype(np.float32) / np.float32(factor * factor)
    if threshold > 0:
        frac = (frac >= np.float32(threshold)).astype(np.float32)
    return frac[:, None]
