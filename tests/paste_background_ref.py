"""Restatement of the pixel-space background paste (include/mkd.h mkd_paste_background; test infrastructure only) in numpy float32,
one numpy operation per rounding."""
import numpy as np


def class_counts(labels: np.ndarray, classes, f: int) -> np.ndarray:
    """labels uint8 [B, f H, f W] -> int64 [B, H, W]: label pixels of each f x f block whose label l < 64 is in ``classes``"""
    B, LH, LW = labels.shape
    assert LH % f == 0 and LW % f == 0
    table = np.zeros(256, bool)
    for c in classes:
        assert 0 <= int(c) < 64
        table[int(c)] = True
    inside = table[labels]
    return inside.reshape(B, LH // f, f, LW // f, f).sum((2, 4)).astype(np.int64)


def window_sums(cnt: np.ndarray, rho: int) -> np.ndarray:
    """sum over the (2 rho + 1)^2 window with indices clamped to the image edge (an edge pixel counts once per clamped offset)"""
    H, W = cnt.shape[-2:]
    off = np.arange(-rho, rho + 1)
    ys = np.clip(np.arange(H)[:, None] + off[None], 0, H - 1)          # [H, win]
    xs = np.clip(np.arange(W)[:, None] + off[None], 0, W - 1)
    rows = cnt[..., ys, :].sum(-2)                                     # [..., H, win, W] -> [..., H, W]
    return rows[..., xs].sum(-1)                                       # [..., H, W, win] -> [..., H, W]


def alpha_from_labels(labels: np.ndarray, classes, f: int, rho: int) -> np.ndarray:
    """-> float32 [B, 1, H, W]: integer counts, ONE correctly rounded division"""
    S = window_sums(class_counts(np.asarray(labels, np.uint8), classes, f), rho)
    D = np.float32((2 * rho + 1) ** 2 * f * f)
    a = S.astype(np.float32) / D
    assert a.dtype == np.float32
    return a[:, None]


def paste(image: np.ndarray, src: np.ndarray, alpha: np.ndarray) -> np.ndarray:
    """image, src float32 [B, C, H, W], alpha float32 [1|B, 1, H, W] -> float32 [B, C, H, W]: the seven operations, one numpy op each"""
    t, s, a = (np.asarray(v, np.float32) for v in (image, src, alpha))
    one, two = np.float32(1.0), np.float32(2.0)
    u = (s + one) / two
    v = (t + one) / two
    p = a * u
    q = (one - a) * v
    r = p + q
    o = r * two - one
    o = np.minimum(np.maximum(o, -one), one)
    assert o.dtype == np.float32
    return o


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
