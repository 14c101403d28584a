"""The teacher on the device: EleGANt's pseudo ground truth (reference teacher.py:96-112, the default ``ELEGANT_PGT`` of
diffmk/makeup_diffuse.py:328-334).  Its first term is the source with its lip, eye and skin regions histogram-matched to the same
regions of the reference (warp weight alpha = 0: pseudo_ground_truth as it always was); its second term, opt-in through ``warp``, blends in
the reference warped onto the source through the landmarks by a thin-plate spline (tps_coefficients on the host, warp_blend on the
device).  Opt-in again (``points='masks'``, ``solve='device'``), the control points come from the region masks instead of landmarks
(region_points) and the spline is solved on the device (tps_coefficients_device): the warped teacher then needs no landmark file and
no host round trip.  The SCGAN / EleGANt generators need external weights and are not here.

Everything but the landmarks takes device tensors and returns device tensors without waiting for the device; the arithmetic is libmkd's
(mkd_region_mask_from_labels, mkd_hist_match, mkd_pgt_compose, mkd_pgt_warp, mkd_region_points, mkd_tps_solve; include/mkd.h has the
definitions, tests/teacher_ref.py, tests/teacher_warp_ref.py and tests/teacher_points_ref.py restate them).  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import lib as _lib
from . import makeup_score as ms

MAX_FEATHER = 8
STRENGTH_KEYS = ('lip', 'eye', 'skin')
MAX_CTRL = 128
REFERENCE_ALPHAS = dict(skin=0.3, eye=0.8, lip=0.1)          # SKIN_ALPHA, EYE_ALPHA, LIP_ALPHA of reference teacher.py:100-106
TPS_RESIDUAL = 1e-6          # px: a spline that misses a landmark by more is dropped (the sample keeps the alpha = 0 image)
POINT_DIRS = (8, 16)          # support directions per region of region_points: K = 4 (D + 1) control points per image
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


def strength_rows(strengths, batch: int, what: str = 'teacher strength') -> Optional[torch.Tensor]:
    """``strengths`` -> fp32 [batch, 4] in the order lip, skin, eye_left, eye_right, or None for all 1.  A dict takes the keys lip, eye
    (both eyes) and skin, each a number or one per sample; a [batch, 4] tensor or array is taken in that order.  Host values outside
    [0, 1] (or not finite) are a ValueError; a tensor that already lives on the device is the caller's to guarantee (looking at it would
    wait for the device)."""
    if strengths is None:
        return None
    if isinstance(strengths, dict):
        extra = [k for k in strengths if k not in STRENGTH_KEYS]
        if extra:
            raise ValueError(f'{what}s take the keys {list(STRENGTH_KEYS)}, got {extra}')
        cols = {}
        for k in STRENGTH_KEYS:
            v = torch.as_tensor(strengths.get(k, 1.0), dtype=torch.float32).detach().cpu().reshape(-1)
            if v.numel() not in (1, batch):
                raise ValueError(f"{what} of '{k}' must be one number or one per sample ({batch}), got {v.numel()}")
            cols[k] = v.expand(batch)
        rows = torch.stack([cols['lip'], cols['skin'], cols['eye'], cols['eye']], 1).contiguous()
    else:
        rows = torch.as_tensor(strengths)
        if tuple(rows.shape) != (batch, 4):
            raise ValueError(f'{what}s must be a dict or [{batch}, 4] (lip, skin, eye_left, eye_right), got {tuple(rows.shape)}')
        if rows.device.type != 'cpu':
            return rows.detach().float().contiguous()
        rows = rows.detach().float().contiguous()
    if not bool(torch.isfinite(rows).all()) or float(rows.min()) < 0.0 or float(rows.max()) > 1.0:
        raise ValueError(f'{what}s must lie in [0, 1]')
    return rows


def alpha_rows(warp, batch: int) -> Optional[torch.Tensor]:
    """``warp`` -> the warp weights alpha as host fp32 [batch, 4] in the order lip, skin, eye_left, eye_right, or None for off.  None /
    False: off; True: REFERENCE_ALPHAS; a dict over lip, eye, skin by the rules of strength_rows (a number or one per sample, in [0, 1],
    else ValueError), a missing key taking its reference value."""
    if warp is None or warp is False:
        return None
    if warp is True:
        warp = {}
    if not isinstance(warp, dict):
        raise ValueError(f'warp must be None, a bool or a dict over {list(STRENGTH_KEYS)}, got {warp!r}')
    extra = [k for k in warp if k not in STRENGTH_KEYS]
    if extra:
        raise ValueError(f'warp weights take the keys {list(STRENGTH_KEYS)}, got {extra}')
    return strength_rows({k: warp.get(k, REFERENCE_ALPHAS[k]) for k in STRENGTH_KEYS}, batch, what='warp weight')


def check_points(points, point_dirs=16, solve='host') -> None:
    """the keywords that choose where the control points and the spline of the warped term come from, or ValueError"""
    if points not in (None, 'masks'):
        raise ValueError(f"points must be None (landmarks) or 'masks' (control points from the region masks), got {points!r}")
    if isinstance(point_dirs, bool) or point_dirs not in POINT_DIRS:
        raise ValueError(f'point_dirs must be one of {POINT_DIRS}, got {point_dirs!r}')
    if solve not in ('host', 'device'):
        raise ValueError(f"solve must be 'host' or 'device', got {solve!r}")


def launches(warp: bool = False, points=None, solve: str = 'host') -> int:
    """Launches of ONE pseudo_ground_truth call, whatever the batch and the feather: 16 = 1 torch copy that concatenates the two label
    maps, 10 for the region masks of the concatenated maps (lip and skin 2 each, the two eyes 3 each), mkd_hist_match_launches(0, 0) = 3
    for the tables (memset, histogram, CDF + table), 1 torch copy that gathers the source half of the masks and mkd_pgt_launches() = 1
    for the composition.  (Host ``strengths`` add one host-to-device copy of 16 B bytes, which is not a launch.)  With ``warp`` 17: one
    mkd_pgt_warp more (the copy that gathers the source half of the masks gathers the reference half too) and three small host-to-device copies (the spline, its
    counts and the warp weights), which are not launches.  With ``warp`` and solve='device' 18: mkd_tps_solve_launches() = 1 more, and
    host landmarks go up in one copy instead of the spline in two (landmarks given as device tensors of another dtype or device add the
    casts that bring them over; float64 tensors on the device add nothing).  With ``warp`` and points='masks' 21: mkd_region_points_launches() = 3
    on the masks the call already has and the one solve; the only copy left is that of the warp weights."""
    check_points(points, solve=solve)
    lib = _lib.load()
    n = 1 + 10 + int(lib.mkd_hist_match_launches(0, 0)) + 1 + int(lib.mkd_pgt_launches())
    if not warp:
        return n
    n += int(lib.mkd_pgt_warp_launches())
    if points == 'masks':
        n += int(lib.mkd_region_points_launches())
    if points == 'masks' or solve == 'device':
        n += int(lib.mkd_tps_solve_launches())
    return n


def _tps_kernel(d2: np.ndarray) -> np.ndarray:
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(d2 > 0, d2 * np.log(d2), 0.0)


def tps_coefficients(lms_src, lms_ref, max_ctrl: Optional[int] = None):
    """The thin-plate splines that carry each sample's source landmarks onto its reference landmarks, as mkd_pgt_warp takes them:
    (ctrl float64 [B, max_ctrl, 2], coef float64 [B, 2, max_ctrl + 3], kcount int32 [B]) HOST arrays; max_ctrl defaults to K.

    lms_src / lms_ref: [B, K, 2] in (y, x) order, host arrays or tensors (a device tensor is brought over with .cpu(), which WAITS for the
    device).  The solve is on the host on purpose: landmarks are host data (the reference loads them from lms/<name>.npy) and the systems
    are (K + 3)^2 with K <= 128.  Per sample: repeated source points are dropped (the first is kept), then float64 numpy.linalg.solve of
    [[U(|c_i - c_j|^2), P], [P^T, 0]] [w; a] = [d; 0] with P = [1, y, x], control points c = source landmarks, targets d = reference
    landmarks, U(s) = s log s.  K_b = 0 -- the sample keeps the alpha = 0 image -- when fewer than 3 points are left, when the solve
    raises (collinear points), when anything is not finite, or when the spline misses a landmark by more than TPS_RESIDUAL = 1e-6 px."""
    def host(a, name):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if a.ndim != 3 or a.shape[2] != 2:
            raise ValueError(f'{name} must be [B, K, 2] in (y, x) order, got {tuple(a.shape)}')
        return a.astype(np.float64)
    ls, lr = host(lms_src, 'lms_src'), host(lms_ref, 'lms_ref')
    if ls.shape != lr.shape:
        raise ValueError(f'lms_src and lms_ref must have one shape, got {ls.shape} and {lr.shape}')
    B, K, _ = ls.shape
    M = K if max_ctrl is None else int(max_ctrl)
    if not 1 <= M <= MAX_CTRL or K > M:
        raise ValueError(f'max_ctrl must lie in max(K, 1) .. {MAX_CTRL}, got {M} for K = {K}')
    ctrl, coef, kcount = np.zeros((B, M, 2)), np.zeros((B, 2, M + 3)), np.zeros(B, dtype=np.int32)
    for b in range(B):
        if not (np.isfinite(ls[b]).all() and np.isfinite(lr[b]).all()):
            continue
        _, first = np.unique(ls[b], axis=0, return_index=True)
        keep = np.sort(first)
        c, d = ls[b][keep], lr[b][keep]
        k = len(keep)
        if k < 3:
            continue
        A = np.zeros((k + 3, k + 3))
        A[:k, :k] = _tps_kernel(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1))
        A[:k, k], A[:k, k + 1:] = 1.0, c
        A[k:, :k] = A[:k, k:].T
        rhs = np.zeros((k + 3, 2))
        rhs[:k] = d
        try:
            sol = np.linalg.solve(A, rhs)
        except np.linalg.LinAlgError:
            continue
        if not np.isfinite(sol).all() or np.abs(A[:k] @ sol - d).max() > TPS_RESIDUAL:
            continue
        ctrl[b, :k], kcount[b] = c, k
        coef[b, :, :k], coef[b, :, M:] = sol[:k].T, sol[k:].T
    return ctrl, coef, kcount


def region_points(masks: torch.Tensor, dirs: int = 16, min_area: int = 4):
    """ONE mkd_region_points: masks uint8 [4,n,H,W] on the device in the order lip, skin, eye_left, eye_right (n may be the 2 B of
    [src | ref]) -> (pts float64 [n,K,2] in (y, x) order, use int32 [n,K], count int32 [n,4]) on the device, K = 4 (dirs + 1): per
    exclusive region (lip, eye_left, eye_right, skin: the ids of mkd_pgt_compose, which is also the order of ``count``) its centroid and
    its ``dirs`` support points; a region of fewer than ``min_area`` pixels has use = 0 and points (0, 0).  Exact, and nothing is read
    back."""
    ms._require_cuda(masks, 'masks')
    if masks.dtype != torch.uint8 or masks.dim() != 4 or masks.shape[0] != 4:
        raise ValueError(f'masks must be uint8 [4,n,H,W], got {masks.dtype} {tuple(masks.shape)}')
    check_points(None, dirs)
    if isinstance(min_area, bool) or int(min_area) != min_area or int(min_area) < 1:
        raise ValueError(f'min_area must be an integer >= 1, got {min_area!r}')
    _, n, H, W = (int(v) for v in masks.shape)
    masks = masks.contiguous()
    K = 4 * (int(dirs) + 1)
    lib = _lib.load()
    pts = torch.empty(n, K, 2, dtype=torch.float64, device=masks.device)
    use = torch.empty(n, K, dtype=torch.int32, device=masks.device)
    count = torch.empty(n, 4, dtype=torch.int32, device=masks.device)
    scratch = torch.empty((int(lib.mkd_region_points_scratch_bytes(max(1, min(n, 65535)))),), device=masks.device, dtype=torch.uint8)
    P = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(masks.device):
        _lib.check(lib.mkd_region_points(P(masks), n, H, W, int(dirs), int(min_area), P(pts), P(use), P(count), P(scratch), C.c_void_p(ms._stream())),
                   'mkd_region_points')
    return pts, use, count


def tps_coefficients_device(pts_src: torch.Tensor, pts_ref: torch.Tensor, use_src: Optional[torch.Tensor] = None,
                            use_ref: Optional[torch.Tensor] = None, max_ctrl: Optional[int] = None):
    """ONE mkd_tps_solve: tps_coefficients on the device.  pts_src / pts_ref [B,K,2] in (y, x) order and use_src / use_ref [B,K] (a pair
    counts where both are non-zero; None: everywhere), all on the device -> (ctrl float64 [B,max_ctrl,2], coef float64 [B,2,max_ctrl+3],
    kcount int32 [B]) on the device, as warp_blend takes them; max_ctrl defaults to K.  The rules are tps_coefficients' (repeated source
    points dropped, K_b = 0 for fewer than 3 points, anything not finite, a vanishing pivot or a residual above TPS_RESIDUAL, here over
    all K_b + 3 rows of the system); the elimination is the library's own (include/mkd.h), so the coefficients agree with the host's to
    rounding, not bit for bit.  Nothing is read back."""
    ms._require_cuda(pts_src, 'pts_src')
    ms._require_cuda(pts_ref, 'pts_ref')
    if pts_src.dim() != 3 or pts_src.shape[2] != 2 or tuple(pts_ref.shape) != tuple(pts_src.shape):
        raise ValueError(f'pts_src and pts_ref must be equal [B,K,2] tensors in (y, x) order, got {tuple(pts_src.shape)} and {tuple(pts_ref.shape)}')
    B, K, _ = (int(v) for v in pts_src.shape)
    M = K if max_ctrl is None else int(max_ctrl)
    if not 1 <= M <= MAX_CTRL or K > M:
        raise ValueError(f'max_ctrl must lie in max(K, 1) .. {MAX_CTRL}, got {M} for K = {K}')
    dev = pts_src.device
    pts_src, pts_ref = pts_src.to(torch.float64).contiguous(), pts_ref.to(torch.float64).contiguous()
    flags = []
    for u, what in ((use_src, 'use_src'), (use_ref, 'use_ref')):
        if u is not None:
            ms._require_cuda(u, what)
            if tuple(u.shape) != (B, K):
                raise ValueError(f'{what} must be [{B},{K}], got {tuple(u.shape)}')
            u = u.to(torch.int32).contiguous()
        flags.append(u)
    ctrl = torch.empty(B, M, 2, dtype=torch.float64, device=dev)
    coef = torch.empty(B, 2, M + 3, dtype=torch.float64, device=dev)
    kcount = torch.empty(B, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mkd_tps_solve(P(pts_src), P(pts_ref), P(flags[0]), P(flags[1]), B, K, M, P(ctrl), P(coef), P(kcount),
                                             C.c_void_p(ms._stream())), 'mkd_tps_solve')
    return ctrl, coef, kcount


def _landmarks(lms_src, lms_ref, batch: int):
    """the landmark arrays of a device solve as float64 [B,K,2] tensors (host arrays are not copied here)"""
    out = []
    for a, name in ((lms_src, 'lms_src'), (lms_ref, 'lms_ref')):
        a = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
        if a.dim() != 3 or a.shape[2] != 2:
            raise ValueError(f'{name} must be [B, K, 2] in (y, x) order, got {tuple(a.shape)}')
        out.append(a.to(torch.float64))
    if tuple(out[0].shape) != tuple(out[1].shape):
        raise ValueError(f'lms_src and lms_ref must have one shape, got {tuple(out[0].shape)} and {tuple(out[1].shape)}')
    if out[0].shape[0] != batch:
        raise ValueError(f'landmarks must be [{batch},K,2], got {tuple(out[0].shape)}')
    if not 1 <= out[0].shape[1] <= MAX_CTRL:
        raise ValueError(f'1 .. {MAX_CTRL} landmarks per sample, got {out[0].shape[1]}')
    return out


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


def warp_blend(xh: torch.Tensor, ref01: torch.Tensor, src_masks: torch.Tensor, ref_masks: torch.Tensor, ctrl: torch.Tensor, coef: torch.Tensor,
               kcount: torch.Tensor, alphas: torch.Tensor, feather: int = 0, out: Optional[torch.Tensor] = None, want_map: bool = False):
    """ONE mkd_pgt_warp: xh (the alpha = 0 image) and ref01 fp32 [B,3,H,W], src_masks / ref_masks uint8 [4,B,H,W] in the order lip, skin,
    eye_left, eye_right, the spline of tps_coefficients on the device (ctrl float64 [B,M,2], coef float64 [B,2,M+3], kcount int32 [B]),
    alphas fp32 [B,4] in mask order -> the blended image fp32 [B,3,H,W]; ``out`` may be xh itself (in place).  want_map: also the map
    float64 [B,2,H,W] = (q_y, q_x), the position in the reference of every source pixel."""
    feather = check_feather(feather)
    for t, what in ((xh, 'xh'), (ref01, 'ref01'), (src_masks, 'src_masks'), (ref_masks, 'ref_masks'), (ctrl, 'ctrl'), (coef, 'coef'),
                    (kcount, 'kcount'), (alphas, 'alphas')):
        ms._require_cuda(t, what)
    if xh.dim() != 4 or xh.shape[1] != 3 or tuple(ref01.shape) != tuple(xh.shape):
        raise ValueError(f'xh and ref01 must be equal [B,3,H,W] tensors, got {tuple(xh.shape)} and {tuple(ref01.shape)}')
    B, _, H, W = (int(v) for v in xh.shape)
    for m, what in ((src_masks, 'src_masks'), (ref_masks, 'ref_masks')):
        if m.dtype != torch.uint8 or tuple(m.shape) != (4, B, H, W):
            raise ValueError(f'{what} must be uint8 [4,{B},{H},{W}], got {m.dtype} {tuple(m.shape)}')
    if ctrl.dtype != torch.float64 or ctrl.dim() != 3 or ctrl.shape[0] != B or ctrl.shape[2] != 2 or not 1 <= ctrl.shape[1] <= MAX_CTRL:
        raise ValueError(f'ctrl must be float64 [{B},M,2] with 1 <= M <= {MAX_CTRL}, got {ctrl.dtype} {tuple(ctrl.shape)}')
    M = int(ctrl.shape[1])
    if coef.dtype != torch.float64 or tuple(coef.shape) != (B, 2, M + 3):
        raise ValueError(f'coef must be float64 [{B},2,{M + 3}], got {coef.dtype} {tuple(coef.shape)}')
    if kcount.dtype != torch.int32 or tuple(kcount.shape) != (B,):
        raise ValueError(f'kcount must be int32 [{B}], got {kcount.dtype} {tuple(kcount.shape)}')
    if tuple(alphas.shape) != (B, 4):
        raise ValueError(f'alphas must be [{B},4], got {tuple(alphas.shape)}')
    if xh.dtype != torch.float32 or not xh.is_contiguous():
        if out is xh:
            raise ValueError('in place needs a contiguous fp32 xh')
        xh = xh.float().contiguous()
    ref01, src_masks, ref_masks = ref01.float().contiguous(), src_masks.contiguous(), ref_masks.contiguous()
    ctrl, coef, kcount, alphas = ctrl.contiguous(), coef.contiguous(), kcount.contiguous(), alphas.float().contiguous()
    if out is None:
        out = torch.empty_like(xh)
    elif out.dtype != torch.float32 or tuple(out.shape) != tuple(xh.shape) or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous fp32 {tuple(xh.shape)} tensor')
    qmap = torch.empty(B, 2, H, W, dtype=torch.float64, device=xh.device) if want_map else None
    P = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    with torch.cuda.device(xh.device):
        _lib.check(_lib.load().mkd_pgt_warp(P(xh), P(ref01), P(src_masks), P(ref_masks), P(ctrl), P(coef), P(kcount), P(alphas), B, H, W, M, feather,
                                            P(out), P(qmap), C.c_void_p(ms._stream())), 'mkd_pgt_warp')
    return (out, qmap) if want_map else out


def pseudo_ground_truth(src01: torch.Tensor, ref01: torch.Tensor, src_seg: torch.Tensor, ref_seg: torch.Tensor, strengths=None,
                        feather: int = 2, classes: Optional[dict] = None, lms_src=None, lms_ref=None, warp=None, points=None,
                        point_dirs: int = 16, solve: str = 'host'):
    """The preliminary transfer x_p of (source, reference) -> (x_p fp32 [B,3,H,W] in [0,1], tables uint8 [4,B,3,256], counts int32
    [4,B,2] = (source, reference) pixels of each region), regions in the order lip, skin, eye_left, eye_right.

    src01 / ref01: [B,3,H,W] in [0,1] on the device; src_seg / ref_seg their label maps; ``classes`` as transfer_score takes it.
    Per pair and region the source is histogram-matched to the reference (mkd_hist_match tables; an empty region on either side
    leaves the source as it is), and the four matches are composed with region priority lip, eye_left, eye_right, skin, strength
    a_r and a (2 feather + 1)^2 box feather that treats what lies outside the image as no region (mkd_pgt_compose, include/mkd.h).
    ``strengths``: see strength_rows; host strengths are uploaded with one small host-to-device copy (pageable memory: the host waits for
    that copy, not for the kernels), a device tensor is used where it is.  ``launches()`` kernel launches per call (16), whatever B; no
    result is read back.

    ``warp`` (see alpha_rows) adds the warped term (warp_blend) through a thin-plate spline whose control points and solve are chosen
    by ``points`` and ``solve``.  points=None, solve='host' (the defaults): the landmarks lms_src / lms_ref, [B,K,2] in (y, x) order,
    solved on the host (tps_coefficients) and uploaded.  solve='device': host landmarks are uploaded (one copy for both arrays) and
    solved on the device (tps_coefficients_device); a landmark tensor that is already a contiguous float64 tensor on the device is used
    where it is, any other device tensor costs the cast or copy that brings it there (launches that launches() does not count).  points='masks': no landmarks (giving them is a ValueError); the control points are region_points of
    the [4, 2 B] masks the call already has, with ``point_dirs`` directions, a pair counting where the region has min_area pixels on BOTH
    sides, and the solve is on the device whatever ``solve`` says: nothing crosses the bus but the warp weights.  launches(warp=True,
    points=, solve=) counts each form."""
    feather = check_feather(feather)
    check_points(points, point_dirs, solve)
    alphas = alpha_rows(warp, int(src01.shape[0]))          # (the warp keywords are checked, and the splines solved, before anything else)
    spline = lms = None
    if alphas is None:
        if points is not None or solve != 'host':
            raise ValueError('points / solve choose the control points of the warped term: they only apply with warp')
    elif points == 'masks':
        if lms_src is not None or lms_ref is not None:
            raise ValueError("points='masks' takes the control points from the region masks: lms_src / lms_ref are not combined with it")
    else:
        if lms_src is None or lms_ref is None:
            raise ValueError('warp needs the landmarks of the source and of the reference: lms_src and lms_ref, [B,K,2] in (y, x) order')
        if solve == 'device':
            lms = _landmarks(lms_src, lms_ref, int(src01.shape[0]))
        else:
            spline = tps_coefficients(lms_src, lms_ref)
            if spline[0].shape[0] != int(src01.shape[0]):
                raise ValueError(f'landmarks must be [{int(src01.shape[0])},K,2], got {tuple(spline[0].shape)}')
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
    if alphas is None:
        src_masks = masks[:, :B].contiguous()
    else:          # the same one copy gathers both halves: [src | ref][region]
        src_masks, ref_masks = masks.view(4, 2, B, H, W).permute(1, 0, 2, 3, 4).contiguous().unbind(0)
    x_p = compose(src01, src_masks, tables, None if rows is None else rows.to(dev), feather)
    if alphas is not None and spline is not None:
        ctrl, coef, kcount = spline
        flat = torch.from_numpy(np.concatenate([ctrl.reshape(-1), coef.reshape(-1)])).to(dev)          # one upload for the spline
        warp_blend(x_p, ref01, src_masks, ref_masks, flat[:ctrl.size].view(ctrl.shape), flat[ctrl.size:].view(coef.shape),
                   torch.from_numpy(kcount).to(dev), alphas.to(dev), feather, out=x_p)
    elif alphas is not None:
        if points == 'masks':          # the halves of ONE call on [region][src | ref] are views: no copy
            pts, use, _ = region_points(masks, point_dirs)
            ctrl, coef, kcount = tps_coefficients_device(pts[:B], pts[B:], use[:B], use[B:])
        else:
            if all(t.device.type == 'cpu' for t in lms):
                lms = torch.stack(lms).to(dev).unbind(0)          # host landmarks: one upload for both arrays
            ctrl, coef, kcount = tps_coefficients_device(lms[0].to(dev), lms[1].to(dev))          # (a tensor on the device is used where it is)
        warp_blend(x_p, ref01, src_masks, ref_masks, ctrl, coef, kcount, alphas.to(dev), feather, out=x_p)
    return x_p, tables, counts
