"""The makeup score on the device: region masks of a face-parsing label map and region-wise histogram matching with its L1
distance (reference diffmk/makeups.py:147-245 calling diffmk/histogram_matching.py:41-66), without gradients.

Everything takes device tensors and returns device tensors without waiting for the device (the one host-to-device copy is the small
index table of makeup_hist_terms / transfer_score, uploaded on the first call for a batch size and kept); the arithmetic is libmkd's
(mkd_region_mask_from_labels, mkd_hist_match): there is no CPU path.  Counts, tables and matched images equal the reference's; a
batch is scored pair by pair (the reference assumes batch 1).  Build-defined cases: an empty region gives the
identity table, matched = 0 and loss 0 (its count says so); an eye box is clipped to the image; images need not be square."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import lib as _lib

REGIONS = ('lip', 'skin', 'eye_left', 'eye_right')
TERMS = ('sr_lip', 'rs_lip', 'sr_skin', 'rs_skin', 'sr_eye_left', 'rs_eye_left', 'sr_eye_right', 'rs_eye_right')
# reference defaults (makeups.py:179-204): lips 7 / 9; skin 1 / 6 / 13; the eye regions are face labels 1 / 6 around labels 4 / 5
LIP_CLASSES, SKIN_CLASSES, FACE_CLASSES, EYE_LEFT_CLASSES, EYE_RIGHT_CLASSES, EYE_MARGIN = (7, 9), (1, 6, 13), (1, 6), (4,), (5,), 10
DEFAULT_LAMBDAS = dict(lip=1.0, skin_1=1.0, skin_2=1.0, eye=1.0)

# (batch size, device) -> index table [n,4] of mkd_hist_match: one per term layout, uploaded once and kept
_terms_index_cache: Dict[Tuple[int, str], torch.Tensor] = {}
_score_index_cache: Dict[Tuple[int, str], torch.Tensor] = {}


def _bits(classes: Iterable[int]) -> int:
    bits = 0
    for c in classes:
        if not 0 <= int(c) < 64:
            raise ValueError(f'class {c} outside 0..63')
        bits |= 1 << int(c)
    return bits


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{what} must be a tensor')
    if t.device.type != 'cuda':
        raise _lib.MkdError(f'{what} must be on a HIP device (the makeup score has no CPU implementation)')


def label_map(seg: torch.Tensor) -> torch.Tensor:
    """[B,H,W], [B,1,H,W] or [B,H,W,1] labels -> contiguous uint8 [B,H,W] (float maps are rounded; no value check: that would sync)"""
    if not isinstance(seg, torch.Tensor):
        raise TypeError('seg must be a tensor')
    if seg.dim() == 4 and seg.shape[1] == 1:
        seg = seg[:, 0]
    elif seg.dim() == 4 and seg.shape[3] == 1:
        seg = seg[..., 0]
    if seg.dim() != 3:
        raise ValueError(f'seg must be [B,H,W], [B,1,H,W] or [B,H,W,1], got {tuple(seg.shape)}')
    if seg.dtype != torch.uint8:
        seg = (seg.round() if seg.is_floating_point() else seg).clamp(0, 255).to(torch.uint8)
    return seg.contiguous()


def region_mask(seg: torch.Tensor, classes: Iterable[int], box_classes: Iterable[int] = (), margin: int = EYE_MARGIN,
                out: Optional[torch.Tensor] = None):
    """One region of a label map -> (mask uint8 [B,H,W], count int32 [B], box int32 [B,4] or None).  box_classes: keep the mask only
    inside the bounding box of those labels grown by ``margin`` pixels per side (clipped to the image); box = (row min, row max,
    col min, col max) before growing."""
    seg = label_map(seg)
    bits, bbits = _bits(classes), _bits(box_classes)
    if margin < 0:
        raise ValueError('margin must be >= 0')
    _require_cuda(seg, 'seg')
    B, H, W = seg.shape
    if out is None:
        out = torch.empty((B, H, W), device=seg.device, dtype=torch.uint8)
    elif tuple(out.shape) != (B, H, W) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != seg.device:
        raise ValueError('out must be a contiguous uint8 [B,H,W] tensor on the device of seg')
    count = torch.empty((B,), device=seg.device, dtype=torch.int32)
    box = torch.empty((B, 4), device=seg.device, dtype=torch.int32) if bbits else None
    with torch.cuda.device(seg.device):
        _lib.check(_lib.load().mkd_region_mask_from_labels(C.c_void_p(seg.data_ptr()), B, H, W, C.c_uint64(bits), C.c_uint64(bbits), int(margin),
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(count.data_ptr()),
                                                           C.c_void_p(box.data_ptr() if box is not None else None), C.c_void_p(_stream())),
                   'mkd_region_mask_from_labels')
    return out, count, box


def _region_masks_packed(seg: torch.Tensor, lip, skin, face, eye_left, eye_right, margin):
    seg = label_map(seg)
    _require_cuda(seg, 'seg')
    B, H, W = seg.shape
    masks = torch.empty((4, B, H, W), device=seg.device, dtype=torch.uint8)
    counts = [region_mask(seg, lip, out=masks[0])[1], region_mask(seg, skin, out=masks[1])[1],
              region_mask(seg, face, eye_left, margin, out=masks[2])[1], region_mask(seg, face, eye_right, margin, out=masks[3])[1]]
    return masks, counts


def region_masks(seg: torch.Tensor, lip: Iterable[int] = LIP_CLASSES, skin: Iterable[int] = SKIN_CLASSES, face: Iterable[int] = FACE_CLASSES,
                 eye_left: Iterable[int] = EYE_LEFT_CLASSES, eye_right: Iterable[int] = EYE_RIGHT_CLASSES, margin: int = EYE_MARGIN):
    """Label map -> ({lip, skin, eye_left, eye_right: uint8 [B,H,W]}, {the same names: int32 [B] pixel counts}).
    get_msk_lip / get_msk_skin / get_msk_eye of the reference; eye_*: ``face`` labels inside the box of the eye's label grown by
    ``margin`` (the eye's own pixels are not in it)."""
    masks, counts = _region_masks_packed(seg, lip, skin, face, eye_left, eye_right, margin)
    return {r: masks[i] for i, r in enumerate(REGIONS)}, {r: counts[i] for i, r in enumerate(REGIONS)}


def _mask_u8(m: torch.Tensor, n_hw) -> torch.Tensor:
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3 or tuple(m.shape[1:]) != tuple(n_hw):
        raise ValueError(f'mask must be [n,H,W] or [n,1,H,W] with H, W = {tuple(n_hw)}, got {tuple(m.shape)}')
    if m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8)
    return m.contiguous()


def histogram_match(dst: torch.Tensor, ref: torch.Tensor, mask_dst: torch.Tensor, mask_ref: torch.Tensor,
                    index: Optional[torch.Tensor] = None, want_matched: bool = True, want_loss: bool = True):
    """n histogram-matching terms in ONE mkd_hist_match call -> (matched [n,3,H,W] fp32 in 0..255 or None, tables uint8 [n,3,256],
    loss fp32 [n] or None, counts int32 [n,2] (dst, ref mask pixels)).

    dst, ref: fp32 [*,3,H,W] in [0,1]; masks [*,H,W] / [*,1,H,W] (non-zero = inside).  index None: term t uses entry t of all four
    (equal leading sizes); else int32 [n,4] on the device = (dst image, ref image, dst mask, ref mask) of each term, which the
    caller guarantees to lie inside the tensors."""
    for t, what in ((dst, 'dst'), (ref, 'ref'), (mask_dst, 'mask_dst'), (mask_ref, 'mask_ref')):
        _require_cuda(t, what)
    if dst.dim() != 4 or ref.dim() != 4 or dst.shape[1] != 3 or ref.shape[1] != 3 or tuple(dst.shape[2:]) != tuple(ref.shape[2:]):
        raise ValueError(f'dst and ref must be [*,3,H,W] with equal H, W, got {tuple(dst.shape)} and {tuple(ref.shape)}')
    H, W = int(dst.shape[2]), int(dst.shape[3])
    if H * W > 1 << 24:
        raise ValueError('H * W must not exceed 2^24 (the counts are compared as fp32)')
    dst, ref = dst.float().contiguous(), ref.float().contiguous()
    mask_dst, mask_ref = _mask_u8(mask_dst, (H, W)), _mask_u8(mask_ref, (H, W))
    if index is None:
        n = int(dst.shape[0])
        if not (ref.shape[0] == mask_dst.shape[0] == mask_ref.shape[0] == n):
            raise ValueError('without an index, dst, ref and both masks need the same number of entries')
    else:
        _require_cuda(index, 'index')
        if index.dim() != 2 or index.shape[1] != 4 or index.dtype != torch.int32:
            raise ValueError('index must be int32 [n,4]')
        index = index.contiguous()
        n = int(index.shape[0])
    if not 1 <= n <= 65535:
        raise ValueError('1 <= n <= 65535 terms per call')
    dev = dst.device
    lib = _lib.load()
    matched = torch.empty((n, 3, H, W), device=dev, dtype=torch.float32) if want_matched else None
    tables = torch.empty((n, 3, 256), device=dev, dtype=torch.uint8)
    loss = torch.empty((n,), device=dev, dtype=torch.float32) if want_loss else None
    counts = torch.empty((n, 2), device=dev, dtype=torch.int32)
    scratch = torch.empty((int(lib.mkd_hist_match_scratch_bytes(n)),), device=dev, dtype=torch.uint8)
    P = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(lib.mkd_hist_match(P(dst), P(ref), P(mask_dst), P(mask_ref), P(index), n, H, W, P(matched), P(tables), P(loss), P(counts),
                                      P(scratch), C.c_void_p(_stream())), 'mkd_hist_match')
    return matched, tables, loss, counts


def _term_index(B: int, device: torch.device) -> torch.Tensor:
    """index rows of the 8 B terms over images [SR | RS | R | S] (4B) and masks [region][src | ref] (4 x 2B); row (2 r + d) B + b"""
    key = (B, str(device))
    if key not in _terms_index_cache:
        rows = []
        for r in range(4):
            for d in range(2):
                for b in range(B):
                    ms, mr = r * 2 * B + b, r * 2 * B + B + b
                    rows.append((b, 2 * B + b, ms, mr) if d == 0 else (B + b, 3 * B + b, mr, ms))
        _terms_index_cache[key] = torch.tensor(rows, dtype=torch.int32).to(device)
    return _terms_index_cache[key]


def makeup_hist_terms(SR: torch.Tensor, RS: torch.Tensor, S: torch.Tensor, R: torch.Tensor, src_seg: torch.Tensor, ref_seg: torch.Tensor,
                      lambdas: Optional[dict] = None, classes: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """The eight histogram terms of p_loss_makeup (makeups.py:147-177) for every pair of a batch, as ONE mkd_hist_match call.

    SR / RS: the transfer results on the source / reference layout, S / R: the real images, all [B,3,H,W] in [0,1]; src_seg / ref_seg
    their label maps.  sr_<region> [B] = lambda * L1(SR, SR matched to R) under (src, ref) masks, rs_<region> = the same for
    (RS, S) under (ref, src) masks.  ``lambdas``: lip, skin_1 (sr_skin), skin_2 (rs_skin), eye (default 1).  Also 'counts'
    int32 [8,B,2] and 'loss_makeup' [B] by the reference's expression, which adds sr_skin twice and rs_skin never (makeups.py:151)."""
    lam = dict(DEFAULT_LAMBDAS)
    lam.update(lambdas or {})
    if set(lam) != set(DEFAULT_LAMBDAS):
        raise ValueError(f'lambdas takes the keys {sorted(DEFAULT_LAMBDAS)}')
    cls = dict(lip=LIP_CLASSES, skin=SKIN_CLASSES, face=FACE_CLASSES, eye_left=EYE_LEFT_CLASSES, eye_right=EYE_RIGHT_CLASSES, margin=EYE_MARGIN)
    cls.update(classes or {})
    for t, what in ((SR, 'SR'), (RS, 'RS'), (S, 'S'), (R, 'R')):
        _require_cuda(t, what)
        if t.dim() != 4 or tuple(t.shape) != tuple(SR.shape) or t.shape[1] != 3:
            raise ValueError(f'SR, RS, S, R must be equal [B,3,H,W] tensors, {what} is {tuple(t.shape)}')
    B, _, H, W = SR.shape
    src_seg, ref_seg = label_map(src_seg), label_map(ref_seg)
    if tuple(src_seg.shape) != (B, H, W) or tuple(ref_seg.shape) != (B, H, W):
        raise ValueError(f'label maps must be [{B},{H},{W}], got {tuple(src_seg.shape)} and {tuple(ref_seg.shape)}')
    dev = SR.device
    imgs = torch.cat([SR.float(), RS.float(), R.float(), S.float()])
    masks, _ = _region_masks_packed(torch.cat([src_seg.to(dev), ref_seg.to(dev)]), cls['lip'], cls['skin'], cls['face'], cls['eye_left'],
                                    cls['eye_right'], cls['margin'])
    flat = masks.view(8 * B, H, W)
    _, _, loss, counts = histogram_match(imgs, imgs, flat, flat, index=_term_index(B, dev), want_matched=False)
    loss = loss.view(8, B)
    w = (lam['lip'], lam['lip'], lam['skin_1'], lam['skin_2'], lam['eye'], lam['eye'], lam['eye'], lam['eye'])
    out = {name: loss[i] * float(w[i]) for i, name in enumerate(TERMS)}
    mk = (out['sr_lip'] + out['rs_lip']) + (out['sr_skin'] + out['sr_skin'])
    mk = mk + (out['sr_eye_left'] + out['rs_eye_left'] + out['sr_eye_right'] + out['rs_eye_right'])
    out['loss_makeup'] = mk * 0.5
    out['counts'] = counts.view(8, B, 2)
    return out


def transfer_score(img: torch.Tensor, ref: torch.Tensor, src_seg: torch.Tensor, ref_seg: torch.Tensor, classes: Optional[dict] = None) -> torch.Tensor:
    """The standard makeup-transfer score of a result -> [B,4] (lip, skin, eye_left, eye_right): per region the L1 distance between
    ``img`` (on the source's layout, [B,3,H,W] in [0,1]) and its histogram match to the makeup reference ``ref``, under the regions
    of src_seg / ref_seg.  One mkd_hist_match call of 4 B terms."""
    cls = dict(lip=LIP_CLASSES, skin=SKIN_CLASSES, face=FACE_CLASSES, eye_left=EYE_LEFT_CLASSES, eye_right=EYE_RIGHT_CLASSES, margin=EYE_MARGIN)
    cls.update(classes or {})
    _require_cuda(img, 'img')
    _require_cuda(ref, 'ref')
    if img.dim() != 4 or img.shape[1] != 3 or tuple(ref.shape) != tuple(img.shape):
        raise ValueError(f'img and ref must be equal [B,3,H,W] tensors, got {tuple(img.shape)} and {tuple(ref.shape)}')
    B, _, H, W = img.shape
    src_seg, ref_seg = label_map(src_seg), label_map(ref_seg)
    if tuple(src_seg.shape) != (B, H, W) or tuple(ref_seg.shape) != (B, H, W):
        raise ValueError(f'label maps must be [{B},{H},{W}], got {tuple(src_seg.shape)} and {tuple(ref_seg.shape)}')
    dev = img.device
    args = (cls['lip'], cls['skin'], cls['face'], cls['eye_left'], cls['eye_right'], cls['margin'])
    ms, _ = _region_masks_packed(src_seg.to(dev), *args)
    mr, _ = _region_masks_packed(ref_seg.to(dev), *args)
    key = (B, str(dev))
    if key not in _score_index_cache:          # row r B + b: (img[b], ref[b], region r of src_seg[b], region r of ref_seg[b])
        _score_index_cache[key] = torch.tensor([(b, b, r * B + b, r * B + b) for r in range(4) for b in range(B)], dtype=torch.int32).to(dev)
    loss = histogram_match(img, ref, ms.view(4 * B, H, W), mr.view(4 * B, H, W), index=_score_index_cache[key], want_matched=False)[2]
    return loss.view(4, B).t().contiguous()
