"""Restatement of the photo calls (include/mkd.h mkd_crop_resize, mkd_resize_coeffs, mkd_paste_photo; test infrastructure only):
Pillow's antialiased bilinear resize of a box in Python doubles and numpy integers, the label sampling, and the paste back in numpy
float32 with one numpy operation per rounding."""
import numpy as np

PRECISION_BITS = 22


def ksize(length: int, S: int) -> int:
    return 2 * max(1, -(-length // S)) + 1


def axis_table(n: int, in0: int, length: int, S: int):
    """-> (bounds int32 [S,2] = (xmin, xmax), coefficients int32 [S, ksize]) of one axis: Python floats are IEEE doubles and every
    operation below rounds once, in the order the header gives"""
    scale = length / S
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    K = ksize(length, S)
    bounds = np.zeros((S, 2), np.int32)
    coef = np.zeros((S, K), np.int32)
    for xx in range(S):
        center = in0 + (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n, int(center + support + 0.5))
        w = []
        for x in range(xmin, xmax):
            a = abs((x - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        assert xmax - xmin <= K
        for i, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            coef[xx, i] = int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coef


def _filter(rows: np.ndarray, bounds: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """rows uint8 [R, N, C] filtered along axis 1 -> uint8 [R, S, C]: clip((2^21 + sum pixel * coef) >> 22) in integers"""
    S = bounds.shape[0]
    out = np.empty((rows.shape[0], S, rows.shape[2]), np.uint8)
    src = rows.astype(np.int64)
    for xx in range(S):
        lo, hi = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + (src[:, lo:hi, :] * coef[xx, :hi - lo].astype(np.int64)[None, :, None]).sum(1)
        assert acc.max(initial=0) < 2 ** 31
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def crop_resize_u8(photo: np.ndarray, box, S: int) -> np.ndarray:
    """photo uint8 [H,W,3], box (x0, y0, w, h) -> uint8 [S,S,3]: horizontal pass over the rows the vertical pass reads, uint8 in
    between, then the vertical pass"""
    H, W = photo.shape[:2]
    x0, y0, bw, bh = box
    bx, cx = axis_table(W, x0, bw, S)
    by, cy = axis_table(H, y0, bh, S)
    first, last = int(by[:, 0].min()), int(by[:, 1].max())
    tmp = _filter(photo[first:last], bx, cx)                                   # [rows, S, 3]
    by = by - first
    return np.ascontiguousarray(_filter(tmp.transpose(1, 0, 2), by, cy).transpose(1, 0, 2))


def img01(u8: np.ndarray) -> np.ndarray:
    """uint8 [S,S,3] -> float32 [3,S,S] = float(u8) / 255.0f"""
    a = u8.astype(np.float32) / np.float32(255.0)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def crop_labels(labels: np.ndarray, box, S: int) -> np.ndarray:
    x0, y0, bw, bh = box
    i = np.arange(S)
    ys = y0 + ((2 * i + 1) * bh) // (2 * S)
    xs = x0 + ((2 * i + 1) * bw) // (2 * S)
    return np.ascontiguousarray(labels[ys[:, None], xs[None, :]])


def _axis(length: int, S: int):
    j = np.arange(length, dtype=np.int64)
    num = (2 * j + 1) * S - length
    den = 2 * length
    i0 = num // den                                      # floor
    rem = num - i0 * den
    w = rem.astype(np.float32) / np.float32(den)
    return np.clip(i0, 0, S - 1), np.clip(i0 + 1, 0, S - 1), w


def feather_alpha(H: int, W: int, box, rho: int) -> np.ndarray:
    """float32 [bh, bw]: float(min(e + 1, rho + 1)) / float(rho + 1), e = distance to the nearest box side not on the photo's border"""
    x0, y0, bw, bh = box
    big = 1 << 30
    j, i = np.arange(bw, dtype=np.int64), np.arange(bh, dtype=np.int64)
    ex = np.full(bw, big, np.int64)
    if x0 > 0:
        ex = np.minimum(ex, j)
    if x0 + bw < W:
        ex = np.minimum(ex, bw - 1 - j)
    ey = np.full(bh, big, np.int64)
    if y0 > 0:
        ey = np.minimum(ey, i)
    if y0 + bh < H:
        ey = np.minimum(ey, bh - 1 - i)
    e = np.minimum(ey[:, None], ex[None, :])
    return np.minimum(e + 1, rho + 1).astype(np.float32) / np.float32(rho + 1)


def paste(photo: np.ndarray, box, t: np.ndarray, s01: np.ndarray, rho: int) -> np.ndarray:
    """photo uint8 [H,W,3], t / s01 float32 [3,S,S] -> the pasted photo (a copy); one numpy float32 operation per rounding"""
    H, W = photo.shape[:2]
    x0, y0, bw, bh = box
    S = t.shape[-1]
    t, s01 = np.asarray(t, np.float32), np.asarray(s01, np.float32)
    r = (t + np.float32(1.0)) * np.float32(0.5)
    d = (r - s01) * np.float32(255.0)
    xa, xb, wx = _axis(bw, S)
    ya, yb, wy = _axis(bh, S)
    wx, wy = wx[None, None, :], wy[None, :, None]
    d00, d01 = d[:, ya][:, :, xa], d[:, ya][:, :, xb]
    d10, d11 = d[:, yb][:, :, xa], d[:, yb][:, :, xb]
    top = d00 + wx * (d01 - d00)
    bot = d10 + wx * (d11 - d10)
    u = top + wy * (bot - top)
    a = feather_alpha(H, W, box, rho)[None]
    region = photo[y0:y0 + bh, x0:x0 + bw].transpose(2, 0, 1).astype(np.float32)
    o = region + a * u
    assert o.dtype == np.float32
    o = np.clip(np.rint(o), np.float32(0.0), np.float32(255.0)).astype(np.uint8)
    out = photo.copy()
    out[y0:y0 + bh, x0:x0 + bw] = o.transpose(1, 2, 0)
    return out
