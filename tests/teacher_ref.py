"""numpy restatement of mkd_pgt_compose (include/mkd.h): the histogram-matching teacher's composition.  It is the definition the kernel
is held to, bit for bit.

  masks  uint8 [4, n, H, W] in the order lip, skin, eye_left, eye_right; tables uint8 [4, n, 3, 256] and strengths [n, 4] in the same order
  id(p)  = the first of lip (1), eye_left (2), eye_right (3), skin (4) whose mask is non-zero at p, else 0
  c_r(p) = the pixels q of the (2 F + 1)^2 window around p that lie inside the image and have id(q) = r;  K = (2 F + 1)^2
  v      = clamp(s, 0, 1) * 255 in fp32 (NaN -> 0, -0 -> +0), i = min(int(v), 255): hist_match_ref.values and its bin
  out    = clamp((v + sum_{r = 1..4} (a_r * (c_r / K)) * (T_r[i] - i)) / 255, 0, 1)
in float64 from the fp32 / integer operands, one operation at a time, the terms added in the order r = 1..4, rounded to fp32 once."""
from __future__ import annotations

import numpy as np

REGIONS = ('lip', 'skin', 'eye_left', 'eye_right')          # the order of the masks, tables and strengths
ID_PLANE = (0, 2, 3, 1)                                     # region id r + 1 -> its plane in that order
MAX_FEATHER = 8


def region_ids(masks: np.ndarray) -> np.ndarray:
    """uint8 [4, ...] masks -> uint8 [...] ids 0..4 by the priority lip, eye_left, eye_right, skin"""
    m = np.asarray(masks) != 0
    ids = np.zeros(m.shape[1:], dtype=np.uint8)
    for r in (3, 2, 1, 0):          # the lowest id is written last: it wins
        ids[m[ID_PLANE[r]]] = r + 1
    return ids


def window_counts(ids: np.ndarray, feather: int) -> np.ndarray:
    """ids [..., H, W] -> int64 [4, ..., H, W]: c_r over the (2 F + 1)^2 window; what lies outside the image counts for no region"""
    F = int(feather)
    H, W = ids.shape[-2:]
    pad = [(0, 0)] * (ids.ndim - 2) + [(F, F), (F, F)]
    out = np.zeros((4,) + ids.shape, dtype=np.int64)
    for r in range(4):
        one = np.pad((ids == r + 1).astype(np.int64), pad)
        for dy in range(2 * F + 1):
            for dx in range(2 * F + 1):
                out[r] += one[..., dy:dy + H, dx:dx + W]
    return out


def values(src: np.ndarray) -> np.ndarray:
    s = np.asarray(src, dtype=np.float32)
    s = np.where(np.isnan(s), np.float32(0), s)
    return (np.clip(s, np.float32(0), np.float32(1)) * np.float32(255) + np.float32(0)).astype(np.float32)          # (+ 0: a zero is +0)


def compose(src, masks, tables, strengths=None, feather: int = 0) -> np.ndarray:
    """src [n, 3, H, W], masks [4, n, H, W], tables [4, n, 3, 256], strengths [n, 4] or None -> fp32 [n, 3, H, W]"""
    src = np.asarray(src, dtype=np.float32)
    n, _, H, W = src.shape
    tables = np.asarray(tables).astype(np.int64)
    a = np.ones((n, 4), dtype=np.float32) if strengths is None else np.asarray(strengths, dtype=np.float32).reshape(n, 4)
    cnt = window_counts(region_ids(masks), feather)                        # [4, n, H, W]
    K = np.float64((2 * int(feather) + 1) ** 2)
    v = values(src)
    i = np.minimum(v.astype(np.int64), 255)
    acc = v.astype(np.float64)
    for r in range(4):
        w = a[:, ID_PLANE[r]].astype(np.float64)[:, None, None] * (cnt[r].astype(np.float64) / K)          # [n, H, W]
        T = np.take_along_axis(tables[ID_PLANE[r]], i.reshape(n, 3, H * W), axis=2).reshape(n, 3, H, W)
        acc = acc + w[:, None] * (T - i).astype(np.float64)
    return np.clip(acc / np.float64(255), 0.0, 1.0).astype(np.float32)


def start_steps(tau: float, steps: int) -> int:
    """the evaluations of a teacher-started pass of ``steps``: k = min(S, max(1, round(tau S))), ties to even (Python's round)"""
    return min(int(steps), max(1, int(round(float(tau) * int(steps)))))


def synthetic_pairs(n: int = 3, size: int = 32, seed: int = 5):
    """n (source, reference) pairs of size x size faces with their label maps: skin 1, eyes 4 / 5, nose 6, lips 7 / 9 on background 0,
    every label a colour of its own (different between source and reference) plus a little noise; the layout moves with the pair.
    -> (src fp32 [n,3,S,S], ref, src_seg uint8 [n,S,S], ref_seg)"""
    rng = np.random.RandomState(seed)
    S = int(size)
    yy, xx = np.mgrid[0:S, 0:S]

    def face(dy, dx):
        seg = np.zeros((S, S), dtype=np.uint8)
        seg[((yy - S / 2 - dy) / (S * 0.44)) ** 2 + ((xx - S / 2 - dx) / (S * 0.38)) ** 2 <= 1.0] = 1
        ey, ex, ly = S * 3 // 8 + dy, S // 4, S * 11 // 16 + dy
        seg[ey:ey + 2, S // 2 + dx - ex - 1:S // 2 + dx - ex + 3] = 4
        seg[ey:ey + 2, S // 2 + dx + ex - 3:S // 2 + dx + ex + 1] = 5
        seg[ey + 3:ly - 2, S // 2 + dx - 1:S // 2 + dx + 2] = 6
        seg[ly:ly + 2, S // 2 + dx - 4:S // 2 + dx + 4] = 7
        seg[ly + 2:ly + 4, S // 2 + dx - 3:S // 2 + dx + 3] = 9
        return seg

    def paint(seg, colours):
        img = np.zeros((3, S, S), dtype=np.float32)
        for lab, col in colours.items():
            img[:, seg == lab] = np.asarray(col, dtype=np.float32)[:, None]
        return np.clip(img + rng.uniform(-0.04, 0.04, img.shape).astype(np.float32), 0, 1).astype(np.float32)

    src_col = {0: (0.1, 0.1, 0.1), 1: (0.75, 0.6, 0.5), 6: (0.7, 0.55, 0.45), 4: (0.2, 0.2, 0.3), 5: (0.2, 0.2, 0.3), 7: (0.6, 0.35, 0.35), 9: (0.6, 0.35, 0.35)}
    ref_col = {0: (0.3, 0.3, 0.4), 1: (0.9, 0.7, 0.65), 6: (0.85, 0.68, 0.6), 4: (0.1, 0.1, 0.1), 5: (0.1, 0.1, 0.1), 7: (0.8, 0.1, 0.2), 9: (0.8, 0.1, 0.2)}
    src, ref, sseg, rseg = [], [], [], []
    for b in range(n):
        s, r = face(b - 1, 1 - b), face(1 - b, b)
        sseg.append(s)
        rseg.append(r)
        src.append(paint(s, src_col))
        ref.append(paint(r, ref_col))
    return np.stack(src), np.stack(ref), np.stack(sseg), np.stack(rseg)


def pseudo_ground_truth(src, ref, src_seg, ref_seg, strengths=None, feather: int = 2):
    """masks -> hist_match_ref tables -> compose, pair by pair -> (x_p [n,3,H,W], tables uint8 [4,n,3,256], counts int64 [4,n,2], masks of
    the source uint8 [4,n,H,W])"""
    import hist_match_ref as href
    n = src.shape[0]
    H, W = src.shape[-2:]
    masks = np.zeros((4, n, H, W), dtype=np.uint8)
    tables = np.zeros((4, n, 3, 256), dtype=np.uint8)
    counts = np.zeros((4, n, 2), dtype=np.int64)
    for b in range(n):
        ms_, mr_ = href.region_masks(src_seg[b]), href.region_masks(ref_seg[b])
        for r, name in enumerate(REGIONS):
            masks[r, b] = ms_[name]
            _, tables[r, b], _, counts[r, b] = href.histogram_match(src[b], ref[b], ms_[name], mr_[name])
    return compose(src, masks, tables, strengths, feather), tables, counts, masks


def transfer_score(img, ref, src_seg, ref_seg) -> np.ndarray:
    """makeup_score.transfer_score on the CPU: [n, 4] losses (lip, skin, eye_left, eye_right)"""
    import hist_match_ref as href
    out = np.zeros((img.shape[0], 4), dtype=np.float32)
    for b in range(img.shape[0]):
        ms_, mr_ = href.region_masks(src_seg[b]), href.region_masks(ref_seg[b])
        for r, name in enumerate(REGIONS):
            out[b, r] = href.histogram_match(img[b], ref[b], ms_[name], mr_[name])[2]
    return out
