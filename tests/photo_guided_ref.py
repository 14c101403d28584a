"""Restatement of the guided pastes (include/mkd.h mkd_paste_photo_guided, mkd_paste_frame_guided; test infrastructure only) on top of
tests/photo_ref.py and tests/photo_frame_ref.py: numpy float32 (box) or float64 (frame), one numpy operation per rounding, in the
header's order, vectorised over photo pixels with a Python loop over the taps.  Also the synthetic edge the tests share."""
import numpy as np

import photo_frame_ref as fr
import photo_ref

RADII = (0, 1, 2)
SIGMA_MIN, SIGMA_MAX = 0.5, 1e6


def model_pixels(t: np.ndarray, s01: np.ndarray):
    """t / s01 float32 [3,S,S] -> (d float32 [3,S,S], Yl float32 [S,S]): the difference of mkd_paste_photo and 256 x the luminance of
    the bytes the model saw"""
    t, s01 = np.asarray(t, np.float32), np.asarray(s01, np.float32)
    r = (t + np.float32(1.0)) * np.float32(0.5)
    d = (r - s01) * np.float32(255.0)
    gb = np.clip(np.rint(s01 * np.float32(255.0)), np.float32(0.0), np.float32(255.0)).astype(np.int64)
    yl = (77 * gb[0] + 150 * gb[1] + 29 * gb[2]).astype(np.float32)
    assert d.dtype == np.float32 and int(yl.max()) <= 65280
    return d, yl


def luma(rgb: np.ndarray) -> np.ndarray:
    """uint8 [...,3] -> int64 77 R + 150 G + 29 B"""
    p = rgb.astype(np.int64)
    return 77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2]


def axis_floor(length: int, S: int):
    """photo_ref._axis with the quotient NOT clamped: (q int64 [length], w float32 [length])"""
    j = np.arange(length, dtype=np.int64)
    num = (2 * j + 1) * S - length
    den = 2 * length
    q = num // den
    return q, (num - q * den).astype(np.float32) / np.float32(den)


def _tent(m: int, w: np.ndarray, inv_t):
    T = w.dtype.type
    dist = T(m) - w if m >= 1 else w + T(-m)
    return T(1.0) - dist * inv_t


def taps(d: np.ndarray, yl: np.ndarray, qy, wy, qx, wx, yh, radius: int, sigma: float, T):
    """u [3, ...] = sum g d / sum g over the (2 R + 2)^2 taps around the unclamped model pixels (qy, qx) with fractions (wy, wx); qy, wy,
    qx, wx and yh broadcast to the shape of the photo pixels; T = np.float32 or np.float64.  -> (u, sw)"""
    S = d.shape[-1]
    R = int(radius)
    assert R in RADII
    if T is np.float32:
        inv = T(1.0) / (T(256.0) * T(sigma))
    else:
        inv = T(1.0) / (T(256.0) * T(np.float32(sigma)))
    inv_t = T(1.0) / T(R + 1)
    dT, ylT = d.astype(T), yl.astype(T)
    wy, wx, yh = wy.astype(T), wx.astype(T), yh.astype(T)
    shape = np.broadcast(qy, qx, yh).shape
    sw = np.zeros(shape, T)
    sc = np.zeros((3,) + shape, T)
    for my in range(-R, R + 2):
        wsy = _tent(my, wy, inv_t)
        ry = np.clip(qy + my, 0, S - 1)
        for mx in range(-R, R + 2):
            wsx = _tent(mx, wx, inv_t)
            rx = np.clip(qx + mx, 0, S - 1)
            q = (yh - ylT[ry, rx]) * inv
            wr = T(1.0) / (T(1.0) + q * q)
            g = (wsy * wsx) * wr
            assert g.dtype == T and q.dtype == T and wr.dtype == T
            sw = sw + g
            sc = sc + g[None] * dT[:, ry, rx]
    assert sw.dtype == T and sc.dtype == T
    assert (sw > 0).all(), 'the weights of a photo pixel vanished'
    u = sc / sw[None]
    assert u.dtype == T
    return u, sw


def paste(photo: np.ndarray, box, t: np.ndarray, s01: np.ndarray, rho: int, radius: int = 1, sigma: float = 8.0, w=None) -> np.ndarray:
    """mkd_paste_photo_guided: photo uint8 [H,W,3], t / s01 float32 [3,S,S], w float32 [wh,ww] or None -> the pasted photo (a copy)"""
    H, W = photo.shape[:2]
    x0, y0, bw, bh = box
    S = t.shape[-1]
    d, yl = model_pixels(t, s01)
    qx, wx = axis_floor(bw, S)
    qy, wy = axis_floor(bh, S)
    region = photo[y0:y0 + bh, x0:x0 + bw]
    yh = luma(region).astype(np.float32)
    u, _ = taps(d, yl, qy[:, None], wy[:, None], qx[None, :], wx[None, :], yh, radius, sigma, np.float32)
    a = photo_ref.feather_alpha(H, W, box, rho)
    if w is not None:
        a = a * plane_at_box(np.asarray(w, np.float32), H, W, box)
    o = region.transpose(2, 0, 1).astype(np.float32) + a[None] * u
    assert o.dtype == np.float32
    out = photo.copy()
    out[y0:y0 + bh, x0:x0 + bw] = np.clip(np.rint(o), np.float32(0.0), np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0)
    return out


def plane_at_box(w: np.ndarray, H: int, W: int, box) -> np.ndarray:
    """mkd_paste_photo_weighted's g: the weight plane float32 [wh,ww] sampled at the box's photo pixels, in float32"""
    x0, y0, bw, bh = box
    xa, xb, ux = (v[x0:x0 + bw] for v in photo_ref._axis(W, w.shape[1]))
    ya, yb, uy = (v[y0:y0 + bh] for v in photo_ref._axis(H, w.shape[0]))
    ux, uy = ux[None, :], uy[:, None]
    lerp = lambda p, q, k: p + k * (q - p)
    g = lerp(lerp(w[ya][:, xa], w[ya][:, xb], ux), lerp(w[yb][:, xa], w[yb][:, xb], ux), uy)
    assert g.dtype == np.float32
    return g


def paste_frame(photo: np.ndarray, frame, t: np.ndarray, s01: np.ndarray, rho: int, radius: int = 1, sigma: float = 8.0, w=None):
    """mkd_paste_frame_guided: frame = (cx, cy, side, c, s) -> (the pasted photo (a copy), o float64 [H,W,3] before rint (the byte itself
    outside the square), inside bool [H,W])"""
    H, W = photo.shape[:2]
    S = t.shape[-1]
    cx, cy, side, c, s = (np.float64(v) for v in frame)
    scale = side / np.float64(S)
    half = side * np.float64(0.5)
    rx = ((np.arange(W, dtype=np.float64) + 0.5) - cx)[None, :]
    ry = ((np.arange(H, dtype=np.float64) + 0.5) - cy)[:, None]
    u = c * rx + s * ry
    v = c * ry - s * rx
    inside = fr.inside_mask(H, W, frame)

    def axis(a):
        g = (a + half) / scale - 0.5
        f = np.floor(g)
        return f.astype(np.int64), g - f
    qx, wx = axis(u)
    qy, wy = axis(v)
    d, yl = model_pixels(t, s01)
    val, _ = taps(d, yl, qy, wy, qx, wx, luma(photo).astype(np.float64), radius, sigma, np.float64)
    e = np.minimum(np.minimum(u + half, half - u), np.minimum(v + half, half - v))
    fr1 = np.float64(rho + 1)
    a = np.minimum(e + 0.5, fr1) / fr1
    if w is not None:
        a = a * fr.plane_at_photo(np.asarray(w, np.float32), H, W)
    byte = photo.transpose(2, 0, 1).astype(np.float64)
    o = np.where(inside[None], byte + a[None] * val, byte).transpose(1, 2, 0)
    out = np.clip(np.rint(o), 0, 255).astype(np.uint8)
    assert np.array_equal(out[~inside], photo[~inside])
    return out, o, inside


# ---- the synthetic edge: a luminance step inside the box, makeup on its bright side only ------------------------------------------------
EDGE_S, EDGE_HW, EDGE_BOX, EDGE_X = 32, 256, (32, 32, 192, 192), 132
EDGE_DARK, EDGE_BRIGHT, EDGE_NOISE, EDGE_LEVELS, EDGE_LUMA = 60, 160, 3, 40, 110 * 256


def edge_case(seed: int = 0):
    """-> (photo uint8 [256,256,3], box, t, s01 float32 [3,32,32]): a grey photo that steps from 60 to 160 at x = 132 (a fractional
    model-pixel position: (132 - 32) 32 / 192 = 16.67) with +-3 noise per byte; s01 is the box's antialiased downsample (photo_ref's
    crop) and t carries +40 / 255 where the model pixel's luminance 77 R + 150 G + 29 B exceeds 110 x 256"""
    g = np.random.default_rng(seed)
    base = np.where(np.arange(EDGE_HW) < EDGE_X, EDGE_DARK, EDGE_BRIGHT)[None, :, None]
    photo = (base + g.integers(-EDGE_NOISE, EDGE_NOISE + 1, (EDGE_HW, EDGE_HW, 3))).astype(np.uint8)
    u8 = photo_ref.crop_resize_u8(photo, EDGE_BOX, EDGE_S)
    s01 = photo_ref.img01(u8)
    bright = luma(u8) > EDGE_LUMA
    r = s01 + np.where(bright, np.float32(EDGE_LEVELS / 255.0), np.float32(0.0))[None].astype(np.float32)
    t = (r * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    return photo, EDGE_BOX, t, s01


def edge_sides(photo: np.ndarray, box):
    """(dark, bright): bool [H,W] masks of the box's pixels left and right of the edge"""
    x0, y0, bw, bh = box
    inbox = np.zeros(photo.shape[:2], bool)
    inbox[y0:y0 + bh, x0:x0 + bw] = True
    left = np.arange(photo.shape[1])[None, :] < EDGE_X
    return inbox & left, inbox & ~left


def edge_figures(before: np.ndarray, after: np.ndarray, box):
    """(summed absolute byte change on the dark side, mean byte change on the bright side)"""
    dark, bright = edge_sides(before, box)
    diff = after.astype(np.int64) - before.astype(np.int64)
    return int(np.abs(diff[dark]).sum()), float(diff[bright].mean())


# ---- the cases tests/test_gpu_photo_guided.py runs on the device and tests/test_photo_guided_host.py runs on the restatement alone --------
CASE_SIZES = (8, 16)
CASE_PHOTO_HW = ((96, 131), (61, 47), (33, 90))
CASE_SIGMAS = (0.5, 8.0, 1e6)
CASE_FEATHERS = (0, 64)
TILE_W, TILE_H = 64, 16                      # the paste kernels' tile: 65 x 17 is one column and one row past it
# (S, radius, sigma, feather, weight plane (wh, ww) or None): every S with every radius and sigma; feathers and planes alternate
CASES = [(S, R, sg, CASE_FEATHERS[(i + j + k) % 2], (None, (7, 11), (40, 33))[(i + 2 * j + k) % 3])
         for i, S in enumerate(CASE_SIZES) for j, R in enumerate(RADII) for k, sg in enumerate(CASE_SIGMAS)]


def case_photos():
    """three photos of differing size: random bytes with a patch of 0 and a patch of 255 each (both clips of the output byte are taken
    from there under t beyond +-1)"""
    g = np.random.default_rng(31007)
    out = []
    for h, w in CASE_PHOTO_HW:
        p = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p[h // 4: h // 2, w // 4: w // 2] = 0
        p[h // 2: 3 * h // 4, w // 2: 3 * w // 4] = 255
        out.append(p)
    return out


def case_boxes(S: int):
    """16 (photo index, box): sizes below S (the window of a tile is then larger than the tile), equal to S, at non-integer ratios,
    1 x 1, one column and one row past the kernel's tile, and x 6; at every photo corner (the taps beyond the model image are clamped
    while their weights are not) and inside"""
    (H0, W0), (H1, W1), (H2, W2) = CASE_PHOTO_HW
    x6 = 6 * S if 6 * S <= H0 else H0
    return [(0, (0, 0, 37, 29)), (0, (W0 - 37, 0, 37, 29)), (0, (0, H0 - 29, 37, 29)), (0, (W0 - 37, H0 - 29, 37, 29)), (0, (41, 30, 37, 29)),
            (0, (17, 0, x6, x6)), (0, (3, H0 - x6, x6, x6)),
            (1, (0, 0, 5, 3)), (1, (W1 - 5, H1 - 3, 5, 3)), (1, (20, 31, 5, 3)), (1, (W1 - 1, H1 - 1, 1, 1)), (1, (0, 0, 1, 1)), (1, (7, 9, S, S)),
            (1, (0, H1 - S, S, S)),
            (2, (11, 7, TILE_W + 1, TILE_H + 1)), (2, (W2 - TILE_W - 1, H2 - TILE_H - 1, TILE_W + 1, TILE_H + 1))]


def case_frames(S: int):
    """16 (photo index, frame): rolls 0, 17 and -40 degrees at four scales with the centre at an odd place inside the photo, and a
    square with a corner beyond each corner of its photo"""
    out = []
    for k in range(12):
        p = k % 3
        H, W = CASE_PHOTO_HW[p]
        out.append((p, fr.frame(W * 0.45 + 0.3141 + k, H * 0.55 + 0.2718 - k, S * (0.6, 1.0, 2.5, 6.0)[k % 4], (0.0, 17.0, -40.0)[(k // 4) % 3])))
    for k, (fx, fy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        p = (k + 1) % 3
        H, W = CASE_PHOTO_HW[p]
        out.append((p, fr.frame(fx * W + (3.377 if fx == 0 else -2.123), fy * H + (1.419 if fy == 0 else -4.733), S * 2.5, (17.0, -40.0, 0.0, 17.0)[k])))
    return out


MISS = fr.frame(-9.9, -9.9, 10.0, 45.0)     # within its side of the photo, but no pixel centre inside: nothing to write


def case_samples(S: int):
    """(t, s01) float32 [16,3,S,S]; t beyond +-1 so that both clips to 0..255 act"""
    g = np.random.default_rng(900 + S)
    s01 = (g.integers(0, 256, (16, 3, S, S)).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    return g.uniform(-3.0, 3.0, s01.shape).astype(np.float32), s01


def case_weights(wt):
    """float32 [16,wh,ww] in [0, 1) with the upper left third at exactly 0 (there the photo's byte stays), or None"""
    if wt is None:
        return None
    w = np.random.default_rng(wt[0] * 100 + wt[1]).random((16,) + tuple(wt)).astype(np.float32)
    w[:, : wt[0] // 3 + 1, : wt[1] // 3 + 1] = 0.0
    return w
