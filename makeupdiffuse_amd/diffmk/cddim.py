"""``diffmk.cddim`` — drop-in for reference diffmk/cddim.py: MKDDIMSampler with denoising_step (:9-79) and
reconstruct (:81-100).  Same names, argument meaning and error behaviour; the arithmetic runs in libmkd."""
from __future__ import annotations

import torch

from ..ddim import *  # noqa: F401,F403  (the reference star-imports the stock sampler module the same way)
from ..ddim import DDIMSampler, np


class MKDDIMSampler(DDIMSampler):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)

    @torch.no_grad()
    def denoising_step(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                       temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                       unconditional_guidance_scale=1., unconditional_conditioning=None, dynamic_threshold=None):
        """One reverse step -> (x_prev, pred_x0).  CFG batches [uncond; cond] through ONE apply_model."""
        return self._step(x, c, t, index, repeat_noise, use_original_steps, quantize_denoised, temperature, noise_dropout,
                          score_corrector, corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning,
                          dynamic_threshold)

    @torch.no_grad()
    def reconstruct(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
                    use_original_steps=False, callback=None):
        """Reverse loop over ddim_timesteps[:t_start], newest first; returns the decoded latent (= DDIMSampler.decode)."""
        return self.decode(x_latent, cond, t_start, unconditional_guidance_scale=unconditional_guidance_scale,
                           unconditional_conditioning=unconditional_conditioning, use_original_steps=use_original_steps,
                           callback=callback)
