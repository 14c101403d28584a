"""Restatement of the tilted-face calls (include/mkd.h mkd_crop_frame, mkd_paste_frame, mkd_face_frames; test infrastructure only) in
numpy float64 / int64: one numpy operation per rounding, in the header's order, vectorised over output pixels with a Python loop over
the taps.  Next to the bytes every function returns the values BEFORE rounding, so that a test can show that none of them lies at a
tie of rint: then the bytes are a condition on the kernel and not on its last bit.  Also the synthetic rolled faces the tests share."""
import math

import numpy as np

UNIT = 16384
INT64_MAX, INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def frame(cx, cy, side, angle_deg):
    """(cx, cy, side, c, s) with exact 0 / +-1 at multiples of 90 degrees (photo.frame_from_box's rule)"""
    q = angle_deg / 90.0
    if q == int(q):
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    else:
        c, s = math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))
    return (float(cx), float(cy), float(side), c, s)


# ---- mkd_crop_frame ------------------------------------------------------------------------------------------------------------------
def crop_frame(photo: np.ndarray, fr, S: int, labels=None):
    """photo uint8 [H,W,3], fr = (cx, cy, side, c, s) -> (u8 uint8 [S,S,3], value float64 [S,S,3] before rint, labels uint8 [S,S] or None)"""
    H, W = photo.shape[:2]
    cx, cy, side, c, s = (np.float64(v) for v in fr)
    scale = side / np.float64(S)
    fs = max(scale, np.float64(1.0))
    half = side * np.float64(0.5)
    R = fs * (abs(c) + abs(s))
    idx = np.arange(S, dtype=np.float64)
    u = ((idx + 0.5) * scale - half)[None, :]
    v = ((idx + 0.5) * scale - half)[:, None]
    qx = (cx + c * u) - s * v
    qy = (cy + s * u) + c * v
    xa, xb = np.floor(qx - R).astype(np.int64), np.floor(qx + R).astype(np.int64)
    ya, yb = np.floor(qy - R).astype(np.int64), np.floor(qy + R).astype(np.int64)
    sw = np.zeros((S, S), np.float64)
    sc = np.zeros((S, S, 3), np.float64)
    src = photo.astype(np.float64)
    for ky in range(int((yb - ya).max()) + 1):
        Y = ya + ky
        dy = (Y.astype(np.float64) + 0.5) - qy
        sdy, cdy = s * dy, c * dy
        Yc = np.clip(Y, 0, H - 1)
        for kx in range(int((xb - xa).max()) + 1):
            X = xa + kx
            dx = (X.astype(np.float64) + 0.5) - qx
            du = c * dx + sdy
            dv = cdy - s * dx
            wu = 1.0 - np.abs(du) / fs
            wv = 1.0 - np.abs(dv) / fs
            on = (wu > 0.0) & (wv > 0.0) & (Y <= yb) & (X <= xb)
            w = np.where(on, wu * wv, 0.0)                       # a tap that is off adds +0.0: no sum changes
            sw = sw + w
            sc = sc + w[..., None] * src[Yc, np.clip(X, 0, W - 1)]
    assert (sw > 0).all()
    value = sc / sw[..., None]
    u8 = np.clip(np.rint(value), 0, 255).astype(np.uint8)
    lab = None
    if labels is not None:
        lab = labels[np.clip(np.floor(qy).astype(np.int64), 0, H - 1), np.clip(np.floor(qx).astype(np.int64), 0, W - 1)]
    return u8, value, lab


def img01(u8: np.ndarray) -> np.ndarray:
    a = u8.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(a.transpose(2, 0, 1))


# ---- mkd_paste_frame -----------------------------------------------------------------------------------------------------------------
def _plane_axis(n_photo: int, n: int):
    X = np.arange(n_photo, dtype=np.int64)
    num = (2 * X + 1) * n - n_photo
    den = 2 * n_photo
    i0 = num // den
    rem = num - i0 * den
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), rem.astype(np.float64) / np.float64(den)


def _lerp(p, q, k):
    return p + k * (q - p)


def plane_at_photo(w: np.ndarray, H: int, W: int) -> np.ndarray:
    """the weight plane float32 [wh,ww] sampled at every photo pixel, in double"""
    wd = w.astype(np.float64)
    xa, xb, ux = _plane_axis(W, w.shape[1])
    ya, yb, uy = _plane_axis(H, w.shape[0])
    ux, uy = ux[None, :], uy[:, None]
    return _lerp(_lerp(wd[ya][:, xa], wd[ya][:, xb], ux), _lerp(wd[yb][:, xa], wd[yb][:, xb], ux), uy)


def inside_mask(H: int, W: int, fr) -> np.ndarray:
    cx, cy, side, c, s = (np.float64(v) for v in fr)
    half = side * np.float64(0.5)
    rx = ((np.arange(W, dtype=np.float64) + 0.5) - cx)[None, :]
    ry = ((np.arange(H, dtype=np.float64) + 0.5) - cy)[:, None]
    u = c * rx + s * ry
    v = c * ry - s * rx
    return (u >= -half) & (u < half) & (v >= -half) & (v < half)


def paste_frame(photo: np.ndarray, fr, t: np.ndarray, s01: np.ndarray, rho: int, w=None):
    """photo uint8 [H,W,3], t / s01 float32 [3,S,S], w float32 [wh,ww] or None -> (the pasted photo (a copy), o float64 [H,W,3] before
    rint (the byte itself outside the square), inside bool [H,W])"""
    H, W = photo.shape[:2]
    S = t.shape[-1]
    cx, cy, side, c, s = (np.float64(v) for v in fr)
    scale = side / np.float64(S)
    half = side * np.float64(0.5)
    rx = ((np.arange(W, dtype=np.float64) + 0.5) - cx)[None, :]
    ry = ((np.arange(H, dtype=np.float64) + 0.5) - cy)[:, None]
    u = c * rx + s * ry
    v = c * ry - s * rx
    inside = (u >= -half) & (u < half) & (v >= -half) & (v < half)

    def axis(a):
        g = (a + half) / scale - 0.5
        f = np.floor(g)
        i0 = f.astype(np.int64)
        return np.clip(i0, 0, S - 1), np.clip(i0 + 1, 0, S - 1), g - f
    c0, c1, wx = axis(u)
    r0, r1, wy = axis(v)
    d = ((t.astype(np.float64) + 1.0) * 0.5 - s01.astype(np.float64)) * 255.0          # [3,S,S]
    top = _lerp(d[:, r0, c0], d[:, r0, c1], wx[None])
    bot = _lerp(d[:, r1, c0], d[:, r1, c1], wx[None])
    val = _lerp(top, bot, wy[None])
    e = np.minimum(np.minimum(u + half, half - u), np.minimum(v + half, half - v))
    fr1 = np.float64(rho + 1)
    a = np.minimum(e + 0.5, fr1) / fr1
    if w is not None:
        a = a * plane_at_photo(w, H, W)
    o = photo.transpose(2, 0, 1).astype(np.float64) + a[None] * val
    o = np.where(inside[None], o, photo.transpose(2, 0, 1).astype(np.float64)).transpose(1, 2, 0)
    out = np.clip(np.rint(o), 0, 255).astype(np.uint8)
    assert np.array_equal(out[~inside], photo[~inside])
    return out, o, inside


def tie_margin(values: np.ndarray) -> float:
    """the smallest distance of a value from a tie of rint (k + 0.5); values clipped away by 0..255 cannot tie"""
    v = np.asarray(values, np.float64)
    v = v[(v > -0.5 - 1e-6) & (v < 255.5 + 1e-6)]
    return float(np.abs((v - np.floor(v)) - 0.5).min()) if v.size else 1.0


# ---- mkd_face_frames -----------------------------------------------------------------------------------------------------------------
def face_frames(labels: np.ndarray, ids: np.ndarray, table: np.ndarray, photo_hw, classes_a=(4,), classes_b=(5,), min_eye_area=None,
                want_exact=False):
    """labels uint8 / ids int32 [B,S,S], table int32 [B,max_out,6], photo_hw [(H, W)] -> int64 [B,max_out,8] rows (n_a, n_b, cq, sq, umin,
    umax, vmin, vmax).  want_exact: also float64 [B,max_out,2], px / len * 16384 and py / len * 16384 before rint (nan where no
    direction was measured)"""
    B, S = labels.shape[0], labels.shape[1]
    K = table.shape[1]
    area = max(1, (S // 128) ** 2) if min_eye_area is None else int(min_eye_area)
    out = np.zeros((B, K, 8), np.int64)
    exact = np.full((B, K, 2), np.nan)
    ys, xs = np.mgrid[0:S, 0:S].astype(np.int64)
    for b in range(B):
        H, W = (int(v) for v in photo_hw[b])
        seen = set()
        for r in range(K):
            cid = int(table[b, r, 0])
            row = [0, 0, UNIT, 0, INT64_MAX, INT64_MIN, INT64_MAX, INT64_MIN]
            if cid >= 0 and cid not in seen:                     # of rows that repeat an id the lowest counts
                seen.add(cid)
                m = ids[b] == cid
                ma, mb = m & np.isin(labels[b], list(classes_a)), m & np.isin(labels[b], list(classes_b))
                na, nb = int(ma.sum()), int(mb.sum())
                row[0], row[1] = na, nb
                if na >= area and nb >= area:
                    px = (np.float64(xs[mb].sum()) / np.float64(nb) - np.float64(xs[ma].sum()) / np.float64(na)) * (np.float64(W) / np.float64(S))
                    py = (np.float64(ys[mb].sum()) / np.float64(nb) - np.float64(ys[ma].sum()) / np.float64(na)) * (np.float64(H) / np.float64(S))
                    if px < 0:
                        px, py = -px, -py
                    ln = np.sqrt(px * px + py * py)
                    if ln != 0:
                        ec, es = px / ln * 16384.0, py / ln * 16384.0
                        exact[b, r] = (ec, es)
                        cq, sq = int(np.rint(ec)), int(np.rint(es))
                        if cq >= UNIT // 2:
                            row[2], row[3] = cq, sq
                cq, sq = row[2], row[3]
                X2, Y2 = (2 * xs[m] + 1) * W, (2 * ys[m] + 1) * H
                pu, pv = cq * X2 + sq * Y2, -sq * X2 + cq * Y2
                if pu.size:
                    row[4:] = [int(pu.min()), int(pu.max()), int(pv.min()), int(pv.max())]
            out[b, r] = row
    return (out, exact) if want_exact else out


# ---- synthetic rolled faces ----------------------------------------------------------------------------------------------------------
def draw_face(labels: np.ndarray, cx: float, cy: float, rx: float, ry: float, roll_deg: float, eyes=(True, True), eye_r: float = None):
    """a skin ellipse (label 1, half-axes rx along the face's right axis and ry along its down axis) rolled by roll_deg about (cx, cy),
    with the two eye blobs (labels 4 and 5; radius 0.25 rx unless eye_r is given: large enough for the centroids of the digitised
    discs to give the roll within a degree) at -+ 0.4 rx along the right axis and 0.25 ry up, drawn into labels [S,S] in place"""
    S = labels.shape[0]
    c, s = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    dx, dy = x + 0.5 - cx, y + 0.5 - cy
    u, v = c * dx + s * dy, -s * dx + c * dy
    labels[(u / rx) ** 2 + (v / ry) ** 2 <= 1.0] = 1
    er = 0.25 * rx if eye_r is None else eye_r
    for on, lab, eu in ((eyes[0], 4, -0.4 * rx), (eyes[1], 5, 0.4 * rx)):
        if on:
            labels[(u - eu) ** 2 + (v + 0.25 * ry) ** 2 <= er * er] = lab
    return labels


TWO_FACES = ((20.0, 24.0, 20.0), (48.0, 44.0, -35.0))          # centre (x, y) on a 64 x 64 map and roll of the two faces below


def two_faces(S: int = 64) -> np.ndarray:
    """two faces on an S x S map, rolled +20 and -35 degrees; the first is the larger"""
    k = S / 64.0
    lab = np.zeros((S, S), np.uint8)
    draw_face(lab, 20 * k, 24 * k, 13 * k, 17 * k, 20.0)
    draw_face(lab, 48 * k, 44 * k, 10 * k, 13 * k, -35.0)
    return lab


# ---- the cases tests/test_gpu_photo_frame.py runs on the device and tests/test_photo_frame_host.py clears of rint ties on the CPU -------
CASE_SIZES = (8, 16, 37)
CASE_PHOTO_HW = ((96, 131), (61, 47), (33, 90))
CASE_ROLLS = (0.0, 17.0, -30.0, 45.0, 90.0)
CASE_SCALES = (0.6, 1.0, 2.5, 7.3)          # side / S: enlarging, 1, reducing
# (S, feather, weight plane (wh, ww) or None): every feather with and without weights, every S
PASTE_CASES = [(CASE_SIZES[k % 3], rho, wt) for k, (rho, wt) in enumerate((r, w) for r in (0, 1, 8, 64) for w in (None, (7, 11)))]
PASTE_CASES[5] = (PASTE_CASES[5][0], PASTE_CASES[5][1], (64, 64))


def case_photos():
    g = np.random.default_rng(20241)
    return [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in CASE_PHOTO_HW]


def case_labels():
    g = np.random.default_rng(20242)
    return [g.integers(0, 19, (h, w), dtype=np.uint8) for h, w in CASE_PHOTO_HW]


def case_frames(S: int):
    """16 (photo index, frame): eleven pairs of CASE_ROLLS x CASE_SCALES with the centre at an odd place inside the photo, a square with
    a corner beyond each corner of its photo, and one whose centre lies outside the photo"""
    out = []
    for k in range(11):
        p = k % 3
        H, W = CASE_PHOTO_HW[p]
        out.append((p, frame(W * 0.45 + 0.3141 + k, H * 0.55 + 0.2718 - k, S * CASE_SCALES[k % 4], CASE_ROLLS[k % 5])))
    for k, (fx, fy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        p = (k + 1) % 3
        H, W = CASE_PHOTO_HW[p]
        out.append((p, frame(fx * W + (3.377 if fx == 0 else -2.123), fy * H + (1.419 if fy == 0 else -4.733), S * 2.5, (17.0, -30.0, 45.0, 17.0)[k])))
    H, W = CASE_PHOTO_HW[0]
    out.append((0, frame(-S * 1.25 * 0.5 + 0.377, H * 0.5 + 0.129, S * 1.25, -30.0)))
    return out


def extra_frames(S: int):
    """single-descriptor calls: the pairs of roll and scale the sixteen above leave out that matter most (the largest support at roll 0
    and 90, a quarter turn while reducing)"""
    H, W = CASE_PHOTO_HW[0]
    return [(0, frame(W * 0.5 + 0.3141, H * 0.5 + 0.2718, S * 7.3, 0.0)), (0, frame(W * 0.4 + 0.77, H * 0.6 + 0.13, S * 7.3, 90.0)),
            (1, frame(20.3141, 30.2718, S * 2.5, 90.0)), (2, frame(40.3141, 15.2718, S * 7.3, 17.0))]


def case_samples(S: int):
    """(t, s01) float32 [16,3,S,S]; t beyond +-1 so that the clip to 0..255 acts"""
    g = np.random.default_rng(500 + S)
    s01 = g.random((16, 3, S, S)).astype(np.float32)
    return g.uniform(-3.0, 3.0, s01.shape).astype(np.float32), s01


def case_weights(wt):
    return None if wt is None else np.random.default_rng(wt[0] * 100 + wt[1]).random((16,) + tuple(wt)).astype(np.float32)


def frames_maps(S: int):
    """(labels uint8 [5,S,S], photo_hw): the two rolled faces behind a square photo; no face; a face without eyes; the two faces behind
    a NON-square photo (the direction is the photo's, not the map's); three faces"""
    k = S / 64.0
    empty = np.zeros((S, S), np.uint8)
    empty[: S // 4, : S // 4] = 12                               # hair: not a face class
    blind = draw_face(np.zeros((S, S), np.uint8), 30 * k, 34 * k, 14 * k, 18 * k, 25.0, eyes=(False, False))
    three = np.zeros((S, S), np.uint8)
    draw_face(three, 14 * k, 16 * k, 10 * k, 13 * k, -12.0)
    draw_face(three, 46 * k, 18 * k, 11 * k, 14 * k, 28.0)
    draw_face(three, 30 * k, 48 * k, 9 * k, 12 * k, 41.0)
    return np.stack([two_faces(S), empty, blind, two_faces(S), three]), [(640, 640), (100, 300), (512, 384), (480, 1100), (777, 333)]
