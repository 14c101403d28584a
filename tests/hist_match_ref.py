"""CPU restatement (numpy) of the reference's region-wise histogram matching: diffmk/histogram_matching.py:41-66 as
diffmk/makeups.py:232-245 (criterionHis) calls it, and the region masks of diffmk/makeups.py:179-230.  tests/golden/hist_match_ref.npz
holds what the reference's own functions gave; test_hist_match_host.py checks this restatement against it, exactly.

One term = (dst image, ref image, dst mask, ref mask), images [3, H, W] in [0, 1]:
  1. v = clamp(x, 0, 1) * 255 in fp32.  Only pixels under the respective mask count.
  2. per channel 256 bins, bin = min(int(v), 255).
  3. pdf = count / total (fp32 division); cdf by sequential fp32 adds.
  4. table[0] = 0, table[255] = 255; table[i] = the first j in 1..255 with cdf_ref[j-1] <= cdf_dst[i] <= cdf_ref[j], else i.
  5. matched = table[int(v)] under the dst mask, 0 elsewhere.
  6. loss = mean over 3 H W of |v mask - matched|.
Build-defined (the reference crashes there): a term with an empty dst or ref mask has the identity table, matched = 0 and loss 0;
an eye box is clipped to the image; images need not be square."""
from __future__ import annotations

import numpy as np

REGIONS = ('lip', 'skin', 'eye_left', 'eye_right')
LIP, SKIN, FACE, EYE_LEFT, EYE_RIGHT, MARGIN = (7, 9), (1, 6, 13), (1, 6), (4,), (5,), 10


def values(x: np.ndarray) -> np.ndarray:
    return (np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.float32)


def cdf(v: np.ndarray) -> np.ndarray:
    """rules 2-3 for the masked values of one channel (1-D fp32, non-empty)"""
    cnt = np.bincount(np.minimum(v.astype(np.int64), 255), minlength=256)
    pdf = cnt.astype(np.float32) / np.float32(cnt.sum())
    return np.add.accumulate(pdf, dtype=np.float32)          # strictly sequential fp32 adds


def table(cdf_dst: np.ndarray, cdf_ref: np.ndarray) -> np.ndarray:
    """rule 4"""
    x = cdf_dst[1:255, None]
    hit = (cdf_ref[None, :255] <= x) & (x <= cdf_ref[None, 1:])          # [254, 255]: column k stands for j = k + 1
    first = hit.argmax(1) + 1
    out = np.arange(256, dtype=np.int64)
    out[1:255] = np.where(hit.any(1), first, out[1:255])
    return out.astype(np.uint8)


def histogram_match(dst, ref, mask_dst, mask_ref):
    """-> (matched [3,H,W] fp32 in 0..255, tables [3,256] uint8, loss fp32, (count_dst, count_ref))"""
    vd, vr = values(dst), values(ref)
    md, mr = np.asarray(mask_dst) != 0, np.asarray(mask_ref) != 0
    nd, nr = int(md.sum()), int(mr.sum())
    tables = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    matched = np.zeros_like(vd)
    if nd == 0 or nr == 0:
        return matched, tables, np.float32(0), (nd, nr)
    for c in range(3):
        tables[c] = table(cdf(vd[c][md]), cdf(vr[c][mr]))
        matched[c][md] = tables[c][np.minimum(vd[c][md].astype(np.int64), 255)].astype(np.float32)
    loss = np.abs(vd * md[None].astype(np.float32) - matched).mean(dtype=np.float32)
    return matched, tables, np.float32(loss), (nd, nr)


def loss_f64(dst, mask_dst, matched) -> float:
    """the float64 mean of |v mask - matched| for a given matched image"""
    vd = values(dst).astype(np.float64) * (np.asarray(mask_dst) != 0)[None]
    return float(np.abs(vd - np.asarray(matched, dtype=np.float64)).mean())


def region_mask(seg: np.ndarray, classes, box_classes=(), margin: int = MARGIN) -> np.ndarray:
    """seg [H,W] integer labels -> uint8 [H,W]: label in classes, and (box_classes given) inside the bounding box of the
    box_classes labels grown by margin on every side, clipped to the image; no such label: empty"""
    seg = np.asarray(seg)
    m = np.isin(seg, list(classes))
    if len(box_classes):
        ys, xs = np.nonzero(np.isin(seg, list(box_classes)))
        box = np.zeros_like(m)
        if ys.size:
            box[max(ys.min() - margin, 0):ys.max() + margin + 1, max(xs.min() - margin, 0):xs.max() + margin + 1] = True
        m &= box
    return m.astype(np.uint8)


def region_masks(seg: np.ndarray) -> dict:
    return {'lip': region_mask(seg, LIP), 'skin': region_mask(seg, SKIN), 'eye_left': region_mask(seg, FACE, EYE_LEFT),
            'eye_right': region_mask(seg, FACE, EYE_RIGHT)}


def makeup_terms(SR, RS, S, R, src_seg, ref_seg) -> dict:
    """the eight unweighted terms of p_loss_makeup for ONE pair: sr_<region> = SR matched to R under (src, ref) masks,
    rs_<region> = RS matched to S under (ref, src) masks"""
    ms, mr = region_masks(src_seg), region_masks(ref_seg)
    out = {}
    for r in REGIONS:
        out['sr_' + r] = histogram_match(SR, R, ms[r], mr[r])[2]
        out['rs_' + r] = histogram_match(RS, S, mr[r], ms[r])[2]
    return out


def loss_makeup(t: dict, lam_lip=1.0, lam_skin_1=1.0, lam_skin_2=1.0, lam_eye=1.0) -> float:
    """diffmk/makeups.py:147-153, literally (the skin bracket doubles sr_skin)"""
    sr_skin = t['sr_skin'] * lam_skin_1
    s = (t['sr_lip'] * lam_lip + t['rs_lip'] * lam_lip) + (sr_skin + sr_skin)
    s += (t['sr_eye_left'] + t['rs_eye_left'] + t['sr_eye_right'] + t['rs_eye_right']) * lam_eye
    return s * 0.5
