"""Region-wise makeup transfer from several references: which region of the face follows which reference, as blend weights of
the ControlNet hint embeddings (include/mkd.h mkd_prepare_regions / mkd_region_weights; BUILD-DEFINED).

User regions are 'eye' (eye_left | eye_right of makeup_score.region_masks), 'lip' and 'skin'.  Where they overlap (the eye boxes lie
inside the skin) a pixel belongs to the first of eye > lip > skin; pixels of no region keep the base hint.  Everything runs on the
device without waiting for it; there is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Mapping, Optional, Sequence, Tuple, Union

import torch

from . import lib as _lib
from . import makeup_score as ms

PRIORITY = ('eye', 'lip', 'skin')
MAX_FEATHER = 4


def ordered(regions: Iterable[str]) -> Tuple[str, ...]:
    """The given user regions in priority order (eye > lip > skin): the order of the weight planes 1.. and of the reference hints."""
    regions = list(regions)
    bad = [r for r in regions if r not in PRIORITY]
    if bad:
        raise ValueError(f'unknown region(s) {bad}: choose from {list(PRIORITY)}')
    if not regions:
        raise ValueError('at least one region is needed')
    if len(set(regions)) != len(regions):
        raise ValueError(f'a region is named twice: {regions}')
    return tuple(r for r in PRIORITY if r in regions)


def strength_rows(strengths: Optional[Mapping[str, Union[float, Sequence[float], torch.Tensor]]], regions: Sequence[str], batch: int):
    """{region: a number or one per sample} -> float32 [batch, K] rows in the order of ``regions`` (host tensor), None when all are 1"""
    if strengths is None:
        return None
    extra = [r for r in strengths if r not in regions]
    if extra:
        raise ValueError(f'strength given for region(s) {extra} that are not transferred ({list(regions)})')
    cols = []
    for r in regions:
        v = torch.as_tensor(strengths.get(r, 1.0), dtype=torch.float32).detach().cpu().reshape(-1)
        if v.numel() not in (1, batch):
            raise ValueError(f"strength of '{r}' must be one number or one per sample ({batch}), got {v.numel()}")
        if not bool(torch.isfinite(v).all()) or float(v.min()) < 0.0:
            raise ValueError(f"strength of '{r}' must be finite and >= 0")
        cols.append(v.expand(batch))
    return torch.stack(cols, 1).contiguous()


def user_region_masks(seg: torch.Tensor, regions: Sequence[str]) -> torch.Tensor:
    """Label map -> uint8 [K, B, H, W] masks of ``regions`` (already in priority order), on the device of seg"""
    masks, _ = ms._region_masks_packed(seg, ms.LIP_CLASSES, ms.SKIN_CLASSES, ms.FACE_CLASSES, ms.EYE_LEFT_CLASSES, ms.EYE_RIGHT_CLASSES,
                                       ms.EYE_MARGIN)                                  # [lip, skin, eye_left, eye_right]
    pick = {'lip': masks[0], 'skin': masks[1]}
    if 'eye' in regions:
        pick['eye'] = masks[2] | masks[3]
    return torch.stack([pick[r] for r in regions]).contiguous()


def region_weights(masks: torch.Tensor, factor: int = 8, feather: int = 1, strength: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mkd_region_weights: masks uint8 [K,B,H,W] on the device -> fp32 [B,K+1,H/factor,W/factor]; strength [B,K] or None."""
    ms._require_cuda(masks, 'masks')
    if masks.dim() != 4 or masks.dtype != torch.uint8:
        raise ValueError(f'masks must be uint8 [K,B,H,W], got {masks.dtype} {tuple(masks.shape)}')
    K, B, H, W = masks.shape
    f, rho = int(factor), int(feather)
    if not 1 <= K <= 7:
        raise ValueError(f'1..7 region masks, got {K}')
    if not 1 <= f <= 64 or H % f or W % f:
        raise ValueError(f'masks {H}x{W} are not a multiple of factor {factor} (1..64)')
    if not 0 <= rho <= MAX_FEATHER:
        raise ValueError(f'feather must be 0..{MAX_FEATHER} latent pixels, got {feather}')
    masks = masks.contiguous()
    st = None
    if strength is not None:
        st = strength.to(device=masks.device, dtype=torch.float32).contiguous()
        if tuple(st.shape) != (B, K):
            raise ValueError(f'strength must be [{B},{K}], got {tuple(st.shape)}')
    out = torch.empty((B, K + 1, H // f, W // f), device=masks.device, dtype=torch.float32)
    with torch.cuda.device(masks.device):
        _lib.check(_lib.load().mkd_region_weights(C.c_void_p(masks.data_ptr()), K, B, H, W, f, rho, C.c_void_p(None if st is None else st.data_ptr()),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   'mkd_region_weights')
    return out


def region_weights_from_seg(seg: torch.Tensor, regions: Iterable[str], factor: int = 8, feather: int = 1,
                            strengths: Optional[Mapping[str, Union[float, Sequence[float], torch.Tensor]]] = None) -> torch.Tensor:
    """Face-parsing label map [B,H,W] (device) -> blend weights fp32 [B, K+1, H/factor, W/factor]: plane 0 the base, plane 1 + i the
    i-th of ``ordered(regions)``.  ``strengths``: {region: a number or one per sample}, missing regions count 1."""
    regs = ordered(regions)
    if not 0 <= int(feather) <= MAX_FEATHER:
        raise ValueError(f'feather must be 0..{MAX_FEATHER} latent pixels, got {feather}')
    seg = ms.label_map(seg)
    st = strength_rows(strengths, regs, int(seg.shape[0]))
    ms._require_cuda(seg, 'seg')
    return region_weights(user_region_masks(seg, regs), factor, feather, None if st is None else st.to(seg.device))
