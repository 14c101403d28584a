"""numpy restatement of mkd_pgt_warp (include/mkd.h): the landmark-warped term of the teacher.  It is the definition the kernel is held
to -- bit for bit where no log reaches the result, within map_tolerance where one does (np.log and the device's log are each within an
ulp, not equal).

  ctrl [n, M, 2] (y, x), coef [n, 2, M + 3] (w_d0 .. w_d,K-1 in front, a_d0 a_d1 a_d2 in the LAST three slots), kcount [n]
  s_k  = (y - c_ky)^2 + (x - c_kx)^2, U(s) = s log(s) for s > 0 else 0
  q_d  = ((sum_k w_dk U(s_k)) + a_d0) + a_d1 y + a_d2 x                         sequential from +0, k = 0 .. K - 1
  m'_r = bilinear sample of (ref mask of region r != 0), a tap outside the image is 0; all 0 unless -1 < q_y < H and -1 < q_x < W
  R_c  = bilinear sample of clamp(ref_c, 0, 1) (NaN -> 0), tap indices clamped to the image
  Wt   = min(1, sum_{r = 1..4} (alpha_r (c_r / Kw)) m'_r),  c_r and Kw = (2 F + 1)^2 as teacher_ref's, from the SOURCE masks
  out  = float32(xh + Wt (R - xh)); the bits of xh where Wt = 0
in float64, one operation at a time, in the order written."""
from __future__ import annotations

import numpy as np

import teacher_ref as tr


def _kernel(s: np.ndarray) -> np.ndarray:
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(s > 0, s * np.log(s), 0.0)


def spline_map(ctrl, coef, kcount, H: int, W: int, want_tolerance: bool = False):
    """-> q float64 [n, 2, H, W]; a sample with K = 0 maps every pixel to itself.  want_tolerance: also tol [n, 2, H, W] =
    2 (K + 8) 2^-52 (sum_k |w_dk U(s_k)| + |a_d0| + |a_d1 y| + |a_d2 x|), a first-order bound of the rounding error of q_d on either side:
    log within 1 ulp, two products per term, a sequential sum of K + 3 terms."""
    ctrl, coef = np.asarray(ctrl, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    n, M = ctrl.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    q = np.zeros((n, 2, H, W))
    tol = np.zeros((n, 2, H, W))
    for b in range(n):
        K = int(kcount[b])
        if K == 0:
            q[b, 0], q[b, 1] = yy, xx
            continue
        acc = [np.zeros((H, W)), np.zeros((H, W))]
        mag = [np.zeros((H, W)), np.zeros((H, W))]
        for k in range(K):
            dy, dx = yy - ctrl[b, k, 0], xx - ctrl[b, k, 1]
            u = _kernel(dy * dy + dx * dx)
            for d in range(2):
                acc[d] = acc[d] + coef[b, d, k] * u
                mag[d] = mag[d] + np.abs(coef[b, d, k] * u)
        for d in range(2):
            a0, a1, a2 = coef[b, d, M], coef[b, d, M + 1], coef[b, d, M + 2]
            q[b, d] = ((acc[d] + a0) + a1 * yy) + a2 * xx
            tol[b, d] = 2.0 * (K + 8) * 2.0 ** -52 * (mag[d] + abs(a0) + np.abs(a1 * yy) + np.abs(a2 * xx))
    return (q, tol) if want_tolerance else q


def _taps(q):
    """q [2, H, W] with -1 < q < size (elsewhere anything) -> y0, x0 (int), fy, fx"""
    y0f, x0f = np.floor(q[0]), np.floor(q[1])
    return y0f.astype(np.int64), x0f.astype(np.int64), q[0] - y0f, q[1] - x0f


def _bilinear(v00, v01, v10, v11, fy, fx):
    top = v00 + fx * (v01 - v00)
    bot = v10 + fx * (v11 - v10)
    return top + fy * (bot - top)


def sample_mask(mask, q, valid):
    """mask [H, W] (non-zero = inside), q [2, H, W] -> m' float64 [H, W]: taps outside the image are 0, not-valid pixels are 0"""
    H, W = mask.shape
    qq = np.where(valid[None], q, 0.0)
    y0, x0, fy, fx = _taps(qq)
    ind = np.pad((np.asarray(mask) != 0).astype(np.float64), 1)          # index + 1: rows / columns -1 and H / W are 0
    v = _bilinear(ind[y0 + 1, x0 + 1], ind[y0 + 1, x0 + 2], ind[y0 + 2, x0 + 1], ind[y0 + 2, x0 + 2], fy, fx)
    return np.where(valid, v, 0.0)


def sample_colour(plane, q, valid):
    """plane fp32 [H, W], q [2, H, W] -> R float64 [H, W] (0 where not valid: unused there)"""
    H, W = plane.shape
    p = np.asarray(plane, dtype=np.float32)
    p = np.clip(np.where(np.isnan(p), np.float32(0), p), np.float32(0), np.float32(1)).astype(np.float64) + 0.0
    qq = np.where(valid[None], q, 0.0)
    y0, x0, fy, fx = _taps(qq)
    ya, yb, xa, xb = np.maximum(y0, 0), np.minimum(y0 + 1, H - 1), np.maximum(x0, 0), np.minimum(x0 + 1, W - 1)
    return _bilinear(p[ya, xa], p[ya, xb], p[yb, xa], p[yb, xb], fy, fx)


def warp(xh, ref, src_masks, ref_masks, ctrl, coef, kcount, alphas, feather: int = 0, want_map: bool = False):
    """xh, ref [n, 3, H, W]; src_masks, ref_masks uint8 [4, n, H, W]; alphas [n, 4] in mask order -> fp32 [n, 3, H, W] (and q)"""
    xh, ref = np.asarray(xh, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    n, _, H, W = xh.shape
    a = np.asarray(alphas, dtype=np.float32).reshape(n, 4)
    cnt = tr.window_counts(tr.region_ids(src_masks), feather)              # [4, n, H, W]
    Kw = np.float64((2 * int(feather) + 1) ** 2)
    q = spline_map(ctrl, coef, kcount, H, W)
    out = xh.copy()
    for b in range(n):
        if int(kcount[b]) == 0:
            continue
        with np.errstate(invalid='ignore'):
            valid = (q[b, 0] > -1.0) & (q[b, 0] < H) & (q[b, 1] > -1.0) & (q[b, 1] < W)
        Wt = np.zeros((H, W))
        for r in range(4):
            w = np.where(cnt[r, b] != 0, np.float64(a[b, tr.ID_PLANE[r]]) * (cnt[r, b].astype(np.float64) / Kw), 0.0)
            Wt = Wt + w * sample_mask(ref_masks[tr.ID_PLANE[r], b], q[b], valid)
        Wt = np.where(Wt < 1.0, Wt, 1.0)
        for c in range(3):
            R = sample_colour(ref[b, c], q[b], valid)
            x = xh[b, c].astype(np.float64)
            out[b, c] = np.where(Wt != 0.0, (x + Wt * (R - x)).astype(np.float32), xh[b, c])
    return (out, q) if want_map else out


def affine_spline(n: int, M: int, rows, K: int = 3, H: int = 8, W: int = 8):
    """a spline with all w = 0: q_d = a_d0 + a_d1 y + a_d2 x with rows = ((a_y0, a_y1, a_y2), (a_x0, a_x1, a_x2)); K control points
    (they do not matter with w = 0) -> ctrl, coef, kcount"""
    ctrl = np.zeros((n, M, 2))
    ctrl[:, :K] = np.stack([np.arange(K) % H, (np.arange(K) * 3) % W], 1)
    coef = np.zeros((n, 2, M + 3))
    coef[:, :, M:] = np.asarray(rows, dtype=np.float64)
    return ctrl, coef, np.full(n, K, dtype=np.int32)


def solve(lms_src, lms_ref, M=None):
    """the standard thin-plate solve in float64 for ONE sample of distinct, non-collinear points (the tests' own; the package's is
    teacher.tps_coefficients) -> ctrl [M, 2], coef [2, M + 3]"""
    c, d = np.asarray(lms_src, dtype=np.float64), np.asarray(lms_ref, dtype=np.float64)
    k = len(c)
    M = k if M is None else M
    A = np.zeros((k + 3, k + 3))
    A[:k, :k] = _kernel(((c[:, None] - c[None]) ** 2).sum(-1))
    A[:k, k], A[:k, k + 1:] = 1.0, c
    A[k:, :k] = A[:k, k:].T
    rhs = np.zeros((k + 3, 2))
    rhs[:k] = d
    sol = np.linalg.solve(A, rhs)
    ctrl, coef = np.zeros((M, 2)), np.zeros((2, M + 3))
    ctrl[:k] = c
    coef[:, :k], coef[:, M:] = sol[:k].T, sol[k:].T
    return ctrl, coef
