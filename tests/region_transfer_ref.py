"""Restatements for the region-wise transfer tests (test infrastructure only; BUILD-DEFINED feature).

  * region_weights: the weight definition of include/mkd.h mkd_region_weights in numpy float32, one rounding per operation;
  * blend_f32: sum_r w_r * e_r in fp32 torch on the given (bf16-valued) embeddings;
  * control_model / apply_model / make_eps_fn: the oracle's ControlNet body (oracle/nets.py control_model) with
    guided = sum_r w[:, r] * hint_block(hint_r) injected, and the eps function the oracle sampler loop takes.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets


def owned_counts(masks: np.ndarray, f: int) -> np.ndarray:
    """masks [K,B,H,W] (non-zero = inside) -> int64 [K,B,H/f,W/f]: pixels of each block owned by k (the lowest k with a non-zero mask)"""
    K, B, H, W = masks.shape
    h, w = H // f, W // f
    nz = masks != 0
    taken = np.zeros((B, H, W), bool)
    cnt = np.zeros((K, B, h, w), np.int64)
    for k in range(K):
        own = nz[k] & ~taken
        taken |= nz[k]
        cnt[k] = own.reshape(B, h, f, w, f).sum((2, 4))
    return cnt


def window_sums(cnt: np.ndarray, rho: int) -> np.ndarray:
    """sum over the (2 rho + 1)^2 window with clamp-to-edge indices (an edge block is counted once per clamped offset)"""
    h, w = cnt.shape[-2:]
    off = np.arange(-rho, rho + 1)
    ys = np.clip(np.arange(h)[:, None] + off[None], 0, h - 1)          # [h, win]
    xs = np.clip(np.arange(w)[:, None] + off[None], 0, w - 1)
    return cnt[..., ys, :][..., xs].sum((-3, -1))                      # [..., h, win, w, win] -> [..., h, w]


def region_weights(masks: np.ndarray, f: int, rho: int, strength=None) -> np.ndarray:
    """-> float32 [B, K+1, h, w]; strength float32 [B, K] or None"""
    K, B = masks.shape[:2]
    S = window_sums(owned_counts(masks, f), rho)
    D = np.float32((2 * rho + 1) ** 2 * f * f)
    wk = S.astype(np.float32) / D                                      # [K,B,h,w], one correctly rounded division
    if strength is not None:
        wk = np.asarray(strength, np.float32).T[:, :, None, None] * wk
    rem = np.ones(wk.shape[1:], np.float32)
    for k in range(K):
        rem = rem - wk[k]
    w0 = np.maximum(np.float32(0.0), rem)
    out = np.concatenate([w0[:, None], wk.transpose(1, 0, 2, 3)], 1)
    assert out.dtype == np.float32
    return out


def blend_f32(es, w: torch.Tensor) -> torch.Tensor:
    """es: R tensors [B, hw, C] (any float dtype), w fp32 [B, R, hw] -> fp32 [B, hw, C]"""
    acc = torch.zeros_like(es[0], dtype=torch.float32)
    for r, e in enumerate(es):
        acc = acc + w[:, r, :, None].float() * e.float()
    return acc


def blend_abs(es, w: torch.Tensor) -> torch.Tensor:
    """sum_r |w_r e_r|: the scale of the per-element bound"""
    acc = torch.zeros_like(es[0], dtype=torch.float32)
    for r, e in enumerate(es):
        acc = acc + (w[:, r, :, None].float() * e.float()).abs()
    return acc


def control_model(sd, cfg, x, hints, weights, timesteps, context, prefix=nets.CONTROL_PREFIX):
    """oracle/nets.py control_model with the region blend: hints R tensors [B,6,8h,8w], weights [B,R,h,w] -> 13 residuals"""
    emb = nets.time_embed(sd, prefix, timesteps, cfg.model_channels)
    guided = None
    for r, hint in enumerate(hints):
        term = weights[:, r:r + 1].to(torch.float32) * nets.hint_block(sd, prefix, hint)
        guided = term if guided is None else guided + term
    outs = []
    h = x
    for i, b in enumerate(nets.encoder_spec(cfg)):
        h = nets._enc_block(sd, cfg, f'{prefix}input_blocks.{i}', b, h, emb, context)
        if i == 0:
            h = h + guided
        outs.append(F.conv2d(h, sd[f'{prefix}zero_convs.{i}.0.weight'], sd[f'{prefix}zero_convs.{i}.0.bias']))
    h = nets._middle(sd, cfg, prefix, h, emb, context)
    outs.append(F.conv2d(h, sd[f'{prefix}middle_block_out.0.weight'], sd[f'{prefix}middle_block_out.0.bias']))
    return outs


def apply_model(sd, cfg, x, t, cond, control_scales=None):
    """oracle/sampler.py apply_model for cond = {'c_crossattn': [ctx], 'c_concat_regions': [hint_0, ...], 'region_weights': w}"""
    ctx = torch.cat(cond['c_crossattn'], 1)
    control = control_model(sd, cfg, x, cond['c_concat_regions'], cond['region_weights'], t, ctx)
    scales = control_scales if control_scales is not None else [1.0] * len(control)
    control = [c * s for c, s in zip(control, scales)]
    return nets.diffusion_model(sd, cfg, x, t, ctx, control=control)


def make_eps_fn(sd, cfg, control_scales=None):
    def fn(x, t, c):
        return apply_model(sd, cfg, x, t, c, control_scales)
    return fn
