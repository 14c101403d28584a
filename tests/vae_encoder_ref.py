"""fp32 CPU restatement of the first-stage ENCODER (test infrastructure only): UPSTREAM ldm Encoder (in_channels 3,
double_z) -> AutoencoderKL.quant_conv -> DiagonalGaussianDistribution -> get_first_stage_encoding, with upstream
state-dict names (first_stage_model.encoder.*, first_stage_model.quant_conv.*).  Configured like oracle.vae.VaeConfig."""
from __future__ import annotations

import zlib
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.vae import PREFIX, VaeConfig, _attn, _gn, _res, _resblock

Tensor = torch.Tensor


def param_spec(cfg: VaeConfig, prefix: str = PREFIX) -> Dict[str, tuple]:
    E = f'{prefix}encoder.'
    d = {f'{E}conv_in.weight': (cfg.ch, 3, 3, 3), f'{E}conv_in.bias': (cfg.ch,)}
    bi = cfg.ch
    for lvl, m in enumerate(cfg.ch_mult):
        bo = cfg.ch * m
        for j in range(cfg.num_res_blocks):
            d.update(_res(f'{E}down.{lvl}.block.{j}', bi, bo))
            bi = bo
        if lvl != len(cfg.ch_mult) - 1:
            d[f'{E}down.{lvl}.downsample.conv.weight'] = (bi, bi, 3, 3)
            d[f'{E}down.{lvl}.downsample.conv.bias'] = (bi,)
    d.update(_res(f'{E}mid.block_1', bi, bi))
    for n in ('q', 'k', 'v', 'proj_out'):
        d[f'{E}mid.attn_1.{n}.weight'] = (bi, bi, 1, 1)
        d[f'{E}mid.attn_1.{n}.bias'] = (bi,)
    d[f'{E}mid.attn_1.norm.weight'] = (bi,)
    d[f'{E}mid.attn_1.norm.bias'] = (bi,)
    d.update(_res(f'{E}mid.block_2', bi, bi))
    d[f'{E}norm_out.weight'] = (bi,)
    d[f'{E}norm_out.bias'] = (bi,)
    d[f'{E}conv_out.weight'] = (2 * cfg.z_channels, bi, 3, 3)
    d[f'{E}conv_out.bias'] = (2 * cfg.z_channels,)
    d[f'{prefix}quant_conv.weight'] = (2 * cfg.embed_dim, 2 * cfg.z_channels, 1, 1)
    d[f'{prefix}quant_conv.bias'] = (2 * cfg.embed_dim,)
    return d


def init_state_dict(cfg: VaeConfig, seed: int = 0, norm_jitter: float = 0.2) -> Dict[str, Tensor]:
    """Seeded synthetic encoder weights, drawn like oracle.vae.init_state_dict."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in sorted(param_spec(cfg).items()):
        if len(shape) == 1:
            if 'norm' in name:
                t = torch.ones(shape) if name.endswith('weight') else torch.zeros(shape)
                if norm_jitter:
                    gn = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(name.encode())) & 0x7FFFFFFF)
                    t = t + norm_jitter * torch.randn(shape, generator=gn)
                sd[name] = t
            else:
                sd[name] = 0.02 * torch.randn(shape, generator=g)
        else:
            fan = 1
            for s in shape[1:]:
                fan *= s
            sd[name] = torch.randn(shape, generator=g) / fan ** 0.5
    return sd


def moments(sd: Dict[str, Tensor], cfg: VaeConfig, x: Tensor, prefix: str = PREFIX) -> Tensor:
    """AutoencoderKL.encode up to the posterior's parameters: Encoder -> quant_conv, [B, 2 embed_dim, H/f, W/f]."""
    E = f'{prefix}encoder.'
    h = F.conv2d(x, sd[f'{E}conv_in.weight'], sd[f'{E}conv_in.bias'], padding=1)
    for lvl in range(len(cfg.ch_mult)):
        for j in range(cfg.num_res_blocks):
            h = _resblock(sd, f'{E}down.{lvl}.block.{j}', h)
        if lvl != len(cfg.ch_mult) - 1:
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), sd[f'{E}down.{lvl}.downsample.conv.weight'],
                         sd[f'{E}down.{lvl}.downsample.conv.bias'], stride=2)
    h = _resblock(sd, f'{E}mid.block_1', h)
    h = _attn(sd, f'{E}mid.attn_1', h)
    h = _resblock(sd, f'{E}mid.block_2', h)
    h = F.silu(_gn(sd, f'{E}norm_out', h))
    h = F.conv2d(h, sd[f'{E}conv_out.weight'], sd[f'{E}conv_out.bias'], padding=1)
    return F.conv2d(h, sd[f'{prefix}quant_conv.weight'], sd[f'{prefix}quant_conv.bias'])


def latent(mom: Tensor, noise: Optional[Tensor] = None, scale_factor: float = 0.18215) -> Tensor:
    """DiagonalGaussianDistribution(mom).sample() with the given noise (None: mode()), x scale_factor."""
    mean, logvar = torch.chunk(mom, 2, dim=1)
    if noise is None:
        return scale_factor * mean
    return scale_factor * (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise)


def ddim_invert(eps_fn, ddim_timesteps, ddim_alphas, ddim_alphas_prev, x0: Tensor, c, t_enc: int) -> Tensor:
    """UPSTREAM DDIMSampler.encode (eta 0, no guidance), fp32, with the model evaluated at ddim_timesteps[i]."""
    x = x0
    for i in range(t_enc):
        a_next, a = float(ddim_alphas[i]), float(ddim_alphas_prev[i])
        t = torch.full((x.shape[0],), int(ddim_timesteps[i]), dtype=torch.long)
        e = eps_fn(x, t, c)
        x = (a_next / a) ** 0.5 * x + a_next ** 0.5 * ((1.0 / a_next - 1.0) ** 0.5 - (1.0 / a - 1.0) ** 0.5) * e
    return x
