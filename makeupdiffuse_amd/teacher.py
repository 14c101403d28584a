"""The histogram-matching teacher on the device: EleGANt's pseudo ground truth (reference teacher.py:96-112, the default
``ELEGANT_PGT`` of diffmk/makeup_diffuse.py:328-334) at warp weight alpha = 0, i.e. the source with its lip, eye and skin regions
histogram-matched to the same regions of the reference.  The landmark-warped term (alpha > 0) and the SCGAN / EleGANt generators need
landmarks and external weights and are not here.

Everything takes device tensors and returns device tensors without waiting for the device; the arithmetic is libmkd's
(mkd_region_mask_from_labels, mkd_hist_match, mkd_pgt_compose; include/mkd.h has the definition, tests/teacher_ref.py restates it).
There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import lib as _lib
from . import makeup_score as ms

MAX_FEATHER = 8
STRENGTH_KEYS = ('lip', 'eye', 'skin')
_index_cache: Dict[Tuple[int, str], torch.Tensor] = {}          # (batch, device) -> the index table of the 4 B terms, uploaded once


def start_steps(tau, steps: int) -> int:
    """The evaluations k of a teacher-started pass of ``steps``: k = min(S, max(1, round(tau S))) with tau in (0, 1] (ties to even,
    Python's round); the pass starts at the sampler's k-th lowest timestep and runs its last k steps."""
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0.0 < float(tau) <= 1.0:
        raise ValueError(f'teacher_start must be a number in (0, 1], got {tau!r}')
    if int(steps) < 1:
        raise ValueError(f'steps must be >= 1, got {steps}')
    return min(int(steps), max(1, int(round(float(tau) * int(steps)))))


def check_feather(feather) -> int:
    if isinstance(feather, bool) or int(feather) != feather or not 0 <= int(feather) <= MAX_FEATHER:
        raise ValueError(f'teacher feather must be an integer in 0..{MAX_FEATHER}, got {feather!r}')
    return int(feather)


def strength_rows(strengths, batch: int) -> Optional[torch.Tensor]:
    """``strengths`` -> fp32 [batch, 4] in the order lip, skin, eye_left, eye_right, or None for all 1.  A dict takes the keys lip, eye
    (both eyes) and skin, each a number or one per sample; a [batch, 4] tensor or array is taken in that order.  Host values outside
    [0, 1] (or not finite) are a ValueError; a tensor that already lives on the device is the caller's to guarantee (looking at it would
    wait for the device)."""
    if strengths is None:
        return None
    if isinstance(strengths, dict):
        extra = [k for k in strengths if k not in STRENGTH_KEYS]
        if extra:
            raise ValueError(f'teacher strengths take the keys {list(STRENGTH_KEYS)}, got {extra}')
        cols = {}
        for k in STRENGTH_KEYS:
            v = torch.as_tensor(strengths.get(k, 1.0), dtype=torch.float32).detach().cpu().reshape(-1)
            if v.numel() not in (1, batch):
                raise ValueError(f"teacher strength of '{k}' must be one number or one per sample ({batch}), got {v.numel()}")
            cols[k] = v.expand(batch)
        rows = torch.stack([cols['lip'], cols['skin'], cols['eye'], cols['eye']], 1).contiguous()
    else:
        rows = torch.as_tensor(strengths)
        if tuple(rows.shape) != (batch, 4):
            raise ValueError(f'teacher strengths must be a dict or [{batch}, 4] (lip, skin, eye_left, eye_right), got {tuple(rows.shape)}')
        if rows.device.type != 'cpu':
            return rows.detach().float().contiguous()
        rows = rows.detach().float().contiguous()
    if not bool(torch.isfinite(rows).all()) or float(rows.min()) < 0.0 or float(rows.max()) > 1.0:
        raise ValueError('teacher strengths must lie in [0, 1]')
    return rows


def launches() -> int:
    """Launches of ONE pseudo_ground_truth call, whatever the batch and the feather: 16 = 1 torch copy that concatenates the two label
    maps, 10 for the region masks of the concatenated maps (lip and skin 2 each, the two eyes 3 each), mkd_hist_match_launches(0, 0) = 3
    for the tables (memset, histogram, CDF + table), 1 torch copy that gathers the source half of the masks and mkd_pgt_launches() = 1
    for the composition.  (Host ``strengths`` add one host-to-device copy of 16 B bytes, which is not a launch.)"""
    lib = _lib.load()
    return 1 + 10 + int(lib.mkd_hist_match_launches(0, 0)) + 1 + int(lib.mkd_pgt_launches())


def compose(src01: torch.Tensor, masks: torch.Tensor, tables: torch.Tensor, strengths: Optional[torch.Tensor] = None, feather: int = 0,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE mkd_pgt_compose: src01 fp32 [B,3,H,W], masks uint8 [4,B,H,W] and tables uint8 [4,B,3,256] in the order lip, skin, eye_left,
    eye_right, strengths fp32 [B,4] on the device or None -> x_p fp32 [B,3,H,W] in [0,1]."""
    feather = check_feather(feather)
    for t, what in ((src01, 'src01'), (masks, 'masks'), (tables, 'tables')):
        ms._require_cuda(t, what)
    if src01.dim() != 4 or src01.shape[1] != 3:
        raise ValueError(f'src01 must be [B,3,H,W], got {tuple(src01.shape)}')
    B, _, H, W = (int(v) for v in src01.shape)
    if masks.dtype != torch.uint8 or tuple(masks.shape) != (4, B, H, W):
        raise ValueError(f'masks must be uint8 [4,{B},{H},{W}], got {masks.dtype} {tuple(masks.shape)}')
    if tables.dtype != torch.uint8 or tuple(tables.shape) != (4, B, 3, 256):
        raise ValueError(f'tables must be uint8 [4,{B},3,256], got {tables.dtype} {tuple(tables.shape)}')
    src01, masks, tables = src01.float().contiguous(), masks.contiguous(), tables.contiguous()
    if strengths is not None:
        ms._require_cuda(strengths, 'strengths')
        if tuple(strengths.shape) != (B, 4):
            raise ValueError(f'strengths must be [{B},4], got {tuple(strengths.shape)}')
        strengths = strengths.float().contiguous()
    if out is None:
        out = torch.empty_like(src01)
    P = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    with torch.cuda.device(src01.device):
        _lib.check(_lib.load().mkd_pgt_compose(P(src01), P(masks), P(tables), P(strengths), B, H, W, feather, P(out), C.c_void_p(ms._stream())),
                   'mkd_pgt_compose')
    return out


def pseudo_ground_truth(src01: torch.Tensor, ref01: torch.Tensor, src_seg: torch.Tensor, ref_seg: torch.Tensor, strengths=None,
                        feather: int = 2, classes: Optional[dict] = None):
    """The preliminary transfer x_p of (source, reference) -> (x_p fp32 [B,3,H,W] in [0,1], tables uint8 [4,B,3,256], counts int32
    [4,B,2] = (source, reference) pixels of each region), regions in the order lip, skin, eye_left, eye_right.

    src01 / ref01: [B,3,H,W] in [0,1] on the device; src_seg / ref_seg their label maps; ``classes`` as transfer_score takes it.
    Per pair and region the source is histogram-matched to the reference (mkd_hist_match tables; an empty region on either side
    leaves the source as it is), and the four matches are composed with region priority lip, eye_left, eye_right, skin, strength
    a_r and a (2 feather + 1)^2 box feather that treats what lies outside the image as no region (mkd_pgt_compose, include/mkd.h).
    ``strengths``: see strength_rows; host strengths are uploaded with one small host-to-device copy (pageable memory: the host waits for
    that copy, not for the kernels), a device tensor is used where it is.  ``launches()`` kernel launches per call (16), whatever B; no
    result is read back."""
    feather = check_feather(feather)
    cls = dict(lip=ms.LIP_CLASSES, skin=ms.SKIN_CLASSES, face=ms.FACE_CLASSES, eye_left=ms.EYE_LEFT_CLASSES, eye_right=ms.EYE_RIGHT_CLASSES,
               margin=ms.EYE_MARGIN)
    cls.update(classes or {})
    ms._require_cuda(src01, 'src01')
    ms._require_cuda(ref01, 'ref01')
    if src01.dim() != 4 or src01.shape[1] != 3 or tuple(ref01.shape) != tuple(src01.shape):
        raise ValueError(f'src01 and ref01 must be equal [B,3,H,W] tensors, got {tuple(src01.shape)} and {tuple(ref01.shape)}')
    B, _, H, W = (int(v) for v in src01.shape)
    rows = strength_rows(strengths, B)
    src_seg, ref_seg = ms.label_map(src_seg), ms.label_map(ref_seg)
    if tuple(src_seg.shape) != (B, H, W) or tuple(ref_seg.shape) != (B, H, W):
        raise ValueError(f'label maps must be [{B},{H},{W}], got {tuple(src_seg.shape)} and {tuple(ref_seg.shape)}')
    dev = src01.device
    src01, ref01 = src01.float().contiguous(), ref01.float().contiguous()
    masks, _ = ms._region_masks_packed(torch.cat([src_seg.to(dev), ref_seg.to(dev)]), cls['lip'], cls['skin'], cls['face'], cls['eye_left'],
                                       cls['eye_right'], cls['margin'])                    # [4, 2B, H, W]: [region][src | ref]
    key = (B, str(dev))
    if key not in _index_cache:          # term r B + b: (source b, reference b, region r of the source, region r of the reference)
        _index_cache[key] = torch.tensor([(b, b, r * 2 * B + b, r * 2 * B + B + b) for r in range(4) for b in range(B)], dtype=torch.int32).to(dev)
    flat = masks.view(8 * B, H, W)
    _, tables, _, counts = ms.histogram_match(src01, ref01, flat, flat, index=_index_cache[key], want_matched=False, want_loss=False)
    tables, counts = tables.view(4, B, 3, 256), counts.view(4, B, 2)
    src_masks = masks[:, :B].contiguous()
    x_p = compose(src01, src_masks, tables, None if rows is None else rows.to(dev), feather)
    return x_p, tables, counts
