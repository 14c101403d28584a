"""Video clips: a sequence of frames made up without flicker.  Three things on top of the photo path (photo.py), none of which changes
an existing call:

* ``FaceTracker``: stable identities for the faces of successive frames, so that a person keeps ONE noise sub-stream for the whole
  clip (noise.Seeds((seed,), (track id,))) however the detector orders or counts the faces of a frame;
* ``smooth_frame``: the crop of a track as a recursively smoothed photo.Frame, so that the model does not see the detector's jitter;
* ``TemporalFilter`` / ``TemporalState`` / ``temporal_diff`` (include/mkd.h mkd_temporal_diff): a motion-aware recursive filter over
  time of the makeup difference d = (t + 1) / 2 - s01 on the device, between the decode and the paste;
* ``MotionSearch`` / ``motion_warp`` (include/mkd.h mkd_motion_warp), off by default: the previous state fetched through one integer
  block-matched vector per block, so that the filter also holds where something moves inside the crop.

``VideoSession`` (TestDiffuseModel.video_session) puts them around the model's single photo pass; ``transfer_video`` feeds it a clip.
The tracker, the smoothing and the slot bookkeeping are host code and need no device; the filter's arithmetic is libmkd's: there is no
CPU path."""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _lib
from . import photo

BETA_MAX = 0.95
TAU_MIN, TAU_MAX = 0.5, 1e6
RADII = (0, 1, 2)
BOX_SMOOTH_MAX = 0.95


# ---- tracks -------------------------------------------------------------------------------------------------------------------------
def region_params(region) -> Tuple[float, float, float, float]:
    """a box (x0, y0, w, h) or a photo.Frame -> (cx, cy, side, angle in degrees); a box's side is its longer one"""
    if len(region) == 5:
        f = photo.Frame(*(float(v) for v in region))
        return f.cx, f.cy, f.side, math.degrees(math.atan2(f.s, f.c))
    if len(region) != 4:
        raise ValueError(f'a region is a box (x0, y0, w, h) or a photo.Frame, got {region!r}')
    x0, y0, bw, bh = (float(v) for v in region)
    if not (bw > 0 and bh > 0):
        raise ValueError(f'box {region!r} is empty')
    return x0 + bw / 2.0, y0 + bh / 2.0, max(bw, bh), 0.0


class FaceTracker:
    """Identities for the faces of successive frames.  ``update(regions)`` takes the faces of ONE frame (boxes or photo.Frame's, in the
    order given; face_parser.find_faces gives them largest first) and returns a track id per face.  The rule is deterministic: for
    each detection in order, among the alive tracks not yet taken in this frame with dist = hypot(dcx, dcy) / side_track <= max_jump
    and max(side / side_track, side_track / side) <= max_scale, the one with the smallest dist wins, ties to the lowest id; the track's
    last RAW detection is what is compared.  No candidate: a new track.  New tracks take ids 0, 1, 2, ... in order of creation and an
    id is never used again.  An unmatched track stays alive for ``max_gap`` further frames, then ends; matched again within them it
    keeps its id -- and so its noise -- but ``restarted`` is True for it: its temporal state and its smoothing start over.
    ``restarted`` (one bool per face of the last update) is also True for a new track."""

    def __init__(self, max_jump: float = 0.5, max_scale: float = 1.5, max_gap: int = 5):
        if not (math.isfinite(float(max_jump)) and float(max_jump) >= 0):
            raise ValueError(f'FaceTracker: max_jump must be a finite number >= 0 (in sides of the track), got {max_jump!r}')
        if not (math.isfinite(float(max_scale)) and float(max_scale) >= 1):
            raise ValueError(f'FaceTracker: max_scale must be a finite ratio >= 1, got {max_scale!r}')
        if isinstance(max_gap, bool) or int(max_gap) != max_gap or int(max_gap) < 0:
            raise ValueError(f'FaceTracker: max_gap must be an integer >= 0 frames, got {max_gap!r}')
        self.max_jump, self.max_scale, self.max_gap = float(max_jump), float(max_scale), int(max_gap)
        self.next_id = 0
        self.frame = 0                                      # frames seen
        self._raw: Dict[int, Tuple[float, float, float, float]] = {}          # alive tracks: id -> the last raw detection
        self._missed: Dict[int, int] = {}                   # ... -> consecutive frames without a match
        self.restarted: List[bool] = []

    @property
    def alive(self) -> List[int]:
        """ids of the alive tracks, ascending"""
        return sorted(self._raw)

    def update(self, regions) -> List[int]:
        taken, ids, restarted = set(), [], []
        for r in regions:
            cx, cy, side, angle = region_params(r)
            best, best_dist = None, math.inf
            for tid in sorted(self._raw):
                if tid in taken:
                    continue
                tx, ty, ts, _ = self._raw[tid]
                dist = math.hypot(cx - tx, cy - ty) / ts
                if dist <= self.max_jump and max(side / ts, ts / side) <= self.max_scale and dist < best_dist:
                    best, best_dist = tid, dist          # (ascending ids and a strict <: ties stay with the lowest id)
            if best is None:
                best = self.next_id
                self.next_id += 1
                restarted.append(True)
            else:
                restarted.append(self._missed[best] > 0)
            taken.add(best)
            self._raw[best] = (cx, cy, side, angle)
            self._missed[best] = 0
            ids.append(best)
        for tid in list(self._raw):
            if tid not in taken:
                self._missed[tid] += 1
                if self._missed[tid] > self.max_gap:
                    del self._raw[tid], self._missed[tid]
        self.frame += 1
        self.restarted = restarted
        return ids


# ---- the crop of a track ------------------------------------------------------------------------------------------------------------
def _wrap180(a: float) -> float:
    """an angle difference in degrees wrapped to (-180, 180]"""
    a = math.fmod(a, 360.0)
    if a > 180.0:
        a -= 360.0
    elif a <= -180.0:
        a += 360.0
    return a


def check_box_smooth(gamma) -> float:
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        g = math.nan
    if isinstance(gamma, bool) or not (0.0 <= g <= BOX_SMOOTH_MAX):
        raise ValueError(f'box_smooth must lie in [0, {BOX_SMOOTH_MAX}], got {gamma!r}')
    return g


def smooth_frame(prev, cur, gamma: float):
    """The crop of a track in this frame: ``cur`` (the raw detection, a box or a photo.Frame) pulled towards ``prev`` (the track's
    SMOOTHED region of the previous frame; None on the first frame of a track).  In double, on p = (cx, cy, ln side, angle) with the
    angle difference wrapped to (-180, 180] degrees: p^ = p + gamma (p^_prev - p).  prev None or gamma 0: ``cur`` itself comes back
    (a box stays the caller's box and takes the crop_resize / paste_photos calls).  Otherwise the result is a photo.Frame, written as
    a correction of ``cur`` (side exp(gamma d ln side), (c, s) turned by gamma d angle), so a constant input is a fixed point bit for
    bit, and an upright frame with integer corners still takes the axis-aligned calls (photo.box_from_frame).  A box must be square
    to be smoothed."""
    g = check_box_smooth(gamma)
    if prev is None or g == 0.0:
        return cur
    if len(cur) == 4:
        if float(cur[2]) != float(cur[3]):
            raise ValueError(f'smooth_frame: box {cur!r} is not square: only a square region can be smoothed into a photo.Frame')
        cur_f = photo.frame_from_box(cur)
    else:
        cur_f = photo.Frame(*(float(v) for v in cur))
    px, py, ps, pa = region_params(prev)
    cx, cy, cs, ca = region_params(cur_f)
    ncx = cx + g * (px - cx)
    ncy = cy + g * (py - cy)
    side = cs * math.exp(g * (math.log(ps) - math.log(cs)))
    turn = math.radians(g * _wrap180(pa - ca))
    ct, st = math.cos(turn), math.sin(turn)
    return photo.Frame(ncx, ncy, side, cur_f.c * ct - cur_f.s * st, cur_f.s * ct + cur_f.c * st)


# ---- the temporal filter ------------------------------------------------------------------------------------------------------------
class TemporalFilter(namedtuple('TemporalFilter', 'beta tau radius')):
    """The temporal filter of the makeup difference (include/mkd.h mkd_temporal_diff).  ``beta`` in (0, 0.95]: the weight of the
    previous frame's filtered difference where nothing moved (the temporal standard deviation of stationary noise falls to
    sqrt((1 - beta) / (1 + beta))); ``tau`` in 8-bit luminance levels (0.5 .. 1e6): the mean absolute luminance change over the window
    at which that weight has fallen to a half; ``radius`` 0, 1 or 2: the window is (2 radius + 1)^2 model pixels."""
    __slots__ = ()

    def __new__(cls, beta: float = 0.8, tau: float = 4.0, radius: int = 1):
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or int(radius) not in RADII:
            raise ValueError(f'TemporalFilter: radius must be 0, 1 or 2, got {radius!r}')
        vals = []
        for v in (beta, tau):
            try:
                vals.append(math.nan if isinstance(v, bool) else float(v))
            except (TypeError, ValueError):
                vals.append(math.nan)
        b, ta = vals
        if not 0.0 < b <= BETA_MAX:
            raise ValueError(f'TemporalFilter: beta must lie in (0, {BETA_MAX}], got {beta!r}')
        if not (math.isfinite(ta) and TAU_MIN <= ta <= TAU_MAX):
            raise ValueError(f'TemporalFilter: tau must be a finite number of luminance levels in [{TAU_MIN}, {TAU_MAX:g}], got {tau!r}')
        return super().__new__(cls, b, ta, int(radius))


def _slots(v, n: int, what: str, who: str = 'temporal_diff'):
    v = [int(x) for x in v]
    if len(v) != n:
        raise ValueError(f'{who}: {what} must hold one slot per face ({n}), got {len(v)}')
    return (C.c_int32 * n)(*v)


def temporal_diff(t: torch.Tensor, s01: torch.Tensor, D_in: torch.Tensor, Y_in: torch.Tensor, slot_in: Sequence[int], D_out: torch.Tensor,
                  Y_out: torch.Tensor, slot_out: Sequence[int], filt: TemporalFilter, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE mkd_temporal_diff launch for the n <= photo.MAX_BATCH faces of a frame step: t, s01 fp32 [n,3,S,S] contiguous on the device;
    the pools D_* [pool,3,S,S] and Y_* [pool,S,S]; face b reads slot slot_in[b] (-1: no previous frame) of the _in pools and writes
    slot slot_out[b] of the _out pools.  Returns the filtered samples, written into ``out`` (default: a new tensor; ``out`` may be
    ``t``).  Everything the library refuses is a lib.MkdError."""
    if not isinstance(filt, TemporalFilter):
        raise ValueError(f'temporal_diff: filt must be a TemporalFilter, got {filt!r}')
    for name, x in (('t', t), ('s01', s01), ('D_in', D_in), ('Y_in', Y_in), ('D_out', D_out), ('Y_out', Y_out)) + ((('out', out),) if out is not None else ()):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f'temporal_diff: {name} must be a contiguous fp32 tensor')
        if x.device.type != 'cuda':
            raise _lib.MkdError(f'temporal_diff: {name} must be on a HIP device (there is no CPU implementation)')
    if t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != t.shape[3] or tuple(s01.shape) != tuple(t.shape):
        raise ValueError(f't and s01 must be [n,3,S,S], got {tuple(t.shape)} and {tuple(s01.shape)}')
    n, S = int(t.shape[0]), int(t.shape[2])
    pool = int(D_in.shape[0]) if D_in.dim() == 4 else -1
    for name, x, shape in (('D_in', D_in, (pool, 3, S, S)), ('Y_in', Y_in, (pool, S, S)), ('D_out', D_out, (pool, 3, S, S)), ('Y_out', Y_out, (pool, S, S))):
        if tuple(x.shape) != shape:
            raise ValueError(f'temporal_diff: {name} must be {list(shape)} (the pools hold the same number of slots), got {tuple(x.shape)}')
    if out is None:
        out = torch.empty_like(t)
    elif tuple(out.shape) != tuple(t.shape):
        raise ValueError(f'temporal_diff: out must have the shape of t {tuple(t.shape)}, got {tuple(out.shape)}')
    p = lambda x: C.c_void_p(x.data_ptr())
    with torch.cuda.device(t.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.load().mkd_temporal_diff(p(t), p(s01), n, S, p(D_in), p(Y_in), _slots(slot_in, n, 'slot_in'), p(D_out), p(Y_out),
                                                 _slots(slot_out, n, 'slot_out'), pool, filt.beta, filt.tau, filt.radius, p(out), st),
                   'mkd_temporal_diff')
    return out


SEARCH_MAX = 7
BLOCKS = (8, 16)
PENALTY_MAX = 65280


class MotionSearch(namedtuple('MotionSearch', 'search block penalty')):
    """Block-matched motion in front of the temporal filter (include/mkd.h mkd_motion_warp).  ``search`` 1..7: a block's displacement
    is looked for among (2 search + 1)^2 integer vectors; ``block`` 8 or 16 model pixels; ``penalty`` 0..65280 in luminance units
    (256 = one grey level) per pixel of the block per pixel of displacement: what a vector must gain over a shorter one."""
    __slots__ = ()

    def __new__(cls, search: int = 3, block: int = 16, penalty: int = 256):
        for name, v in (('search', search), ('block', block), ('penalty', penalty)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f'MotionSearch: {name} must be an integer, got {v!r}')
        if not 1 <= int(search) <= SEARCH_MAX:
            raise ValueError(f'MotionSearch: search must be 1..{SEARCH_MAX} model pixels, got {search!r}')
        if int(block) not in BLOCKS:
            raise ValueError(f'MotionSearch: block must be 8 or 16 model pixels, got {block!r}')
        if not 0 <= int(penalty) <= PENALTY_MAX:
            raise ValueError(f'MotionSearch: penalty must be 0..{PENALTY_MAX} luminance units, got {penalty!r}')
        return super().__new__(cls, int(search), int(block), int(penalty))


def motion_warp(s01: torch.Tensor, D_in: torch.Tensor, Y_in: torch.Tensor, slot_in: Sequence[int], D_w: torch.Tensor, Y_w: torch.Tensor,
                ms: MotionSearch, vec_out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """ONE mkd_motion_warp launch for the n <= photo.MAX_BATCH faces of a frame step: s01 fp32 [n,3,S,S] contiguous on the device; the
    pools D_* [pool,3,S,S] and Y_* [pool,S,S]; face b reads slot slot_in[b] of the _in pools through its blocks' vectors and writes the
    SAME slot of D_w / Y_w (-1: no previous frame, nothing read or written).  ``vec_out``: int32 [n, nb, nb, 2] = (vy, vx) per block,
    nb = ceil(S / block), or None.  Returns ``vec_out``.  Everything the library refuses is a lib.MkdError."""
    if not isinstance(ms, MotionSearch):
        raise ValueError(f'motion_warp: ms must be a MotionSearch, got {ms!r}')
    for name, x in (('s01', s01), ('D_in', D_in), ('Y_in', Y_in), ('D_w', D_w), ('Y_w', Y_w)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f'motion_warp: {name} must be a contiguous fp32 tensor')
        if x.device.type != 'cuda':
            raise _lib.MkdError(f'motion_warp: {name} must be on a HIP device (there is no CPU implementation)')
    if s01.dim() != 4 or s01.shape[1] != 3 or s01.shape[2] != s01.shape[3]:
        raise ValueError(f's01 must be [n,3,S,S], got {tuple(s01.shape)}')
    n, S = int(s01.shape[0]), int(s01.shape[2])
    pool = int(D_in.shape[0]) if D_in.dim() == 4 else -1
    for name, x, shape in (('D_in', D_in, (pool, 3, S, S)), ('Y_in', Y_in, (pool, S, S)), ('D_w', D_w, (pool, 3, S, S)), ('Y_w', Y_w, (pool, S, S))):
        if tuple(x.shape) != shape:
            raise ValueError(f'motion_warp: {name} must be {list(shape)} (the pools hold the same number of slots), got {tuple(x.shape)}')
    if vec_out is not None:
        nb = -(-S // ms.block)
        if not isinstance(vec_out, torch.Tensor) or vec_out.dtype != torch.int32 or not vec_out.is_contiguous() or tuple(vec_out.shape) != (n, nb, nb, 2):
            raise ValueError(f'motion_warp: vec_out must be a contiguous int32 tensor [{n}, {nb}, {nb}, 2]')
        if vec_out.device.type != 'cuda':
            raise _lib.MkdError('motion_warp: vec_out must be on a HIP device')
    p = lambda x: C.c_void_p(None if x is None else x.data_ptr())
    with torch.cuda.device(s01.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.load().mkd_motion_warp(p(s01), n, S, p(D_in), p(Y_in), _slots(slot_in, n, 'slot_in', 'motion_warp'), pool, ms.search, ms.block, ms.penalty,
                                               p(D_w), p(Y_w), p(vec_out), st), 'mkd_motion_warp')
    return vec_out


class SlotPlan:
    """The slot bookkeeping of a TemporalState, host only: which slot of the ``_in`` pools holds the state of a track after the last
    frame step.  ``assign(ids, restarted)`` -> (slot_in, slot_out) of this step: face j writes slot j; it reads the slot it wrote in
    the PREVIOUS step, or -1 when it has none (a new track, one that was not in the previous frame, one marked restarted)."""

    def __init__(self):
        self.held: Dict[int, int] = {}

    def assign(self, ids: Sequence[int], restarted: Optional[Sequence[bool]] = None) -> Tuple[List[int], List[int]]:
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids):
            raise ValueError(f'a track appears once per frame, got {ids}')
        fresh = [False] * len(ids) if restarted is None else [bool(v) for v in restarted]
        if len(fresh) != len(ids):
            raise ValueError(f'{len(ids)} tracks but {len(fresh)} restart flags')
        slot_in = [-1 if f else self.held.get(i, -1) for i, f in zip(ids, fresh)]
        slot_out = list(range(len(ids)))
        self.held = dict(zip(ids, slot_out))
        return slot_in, slot_out


class TemporalState:
    """The state of a TemporalFilter over a clip: the two pools of mkd_temporal_diff (the filtered difference D [pool,3,S,S] and the
    luminance Y [pool,S,S] of every track's last frame), which it sizes to ``capacity`` slots -- the alive tracks -- and grows by
    reallocation, the slots (SlotPlan) and the swap of the pools after every frame.  ``step`` is one frame.  With ``motion`` (a
    MotionSearch) it owns a third pair of pools as well: every step first fetches the previous state through block-matched vectors
    (motion_warp) and the filter reads that; ``motion_launches`` counts those launches, ``last_vectors`` keeps the last step's."""

    def __init__(self, filt: TemporalFilter, size: int, device, capacity: int = 4, motion: Optional[MotionSearch] = None):
        if not isinstance(filt, TemporalFilter):
            raise ValueError(f'TemporalState: filt must be a TemporalFilter, got {filt!r}')
        if motion is not None and not isinstance(motion, MotionSearch):
            raise ValueError(f'TemporalState: motion must be a MotionSearch or None, got {motion!r}')
        self.filt, self.S, self.device, self.motion = filt, photo._check_size(size), torch.device(device), motion
        self.plan = SlotPlan()
        self.capacity = 0
        self.launches = 0
        self.motion_launches = 0
        self.last_vectors: Optional[torch.Tensor] = None          # with motion: int32 [n, nb, nb, 2] = (vy, vx) of the last step's faces
        self._in = self._out = self._warp = None
        self._grow(max(1, int(capacity)))

    def _grow(self, capacity: int) -> None:
        new = lambda: (torch.zeros((capacity, 3, self.S, self.S), device=self.device), torch.zeros((capacity, self.S, self.S), device=self.device))
        nin, nout = new(), new()
        if self._in is not None:          # what the tracks hold lives in the _in pools
            nin[0][:self.capacity].copy_(self._in[0])
            nin[1][:self.capacity].copy_(self._in[1])
        self._in, self._out, self.capacity = nin, nout, capacity
        if self.motion is not None:       # the third pair: the _in pools fetched through the vectors (rewritten in every step)
            self._warp = new()

    def step(self, ids: Sequence[int], t: Optional[torch.Tensor], s01: Optional[torch.Tensor], restarted: Optional[Sequence[bool]] = None,
             alive: int = 0) -> Optional[torch.Tensor]:
        """one frame: the faces ``ids`` (distinct track ids) with their decoded samples t and crops s01 [n,3,S,S] -> the filtered
        samples (a new tensor).  A frame without a face (ids empty, t / s01 unused) is a step too: every track loses its state.
        ``alive``: the number of alive tracks, a lower bound of the pools' size."""
        n = len(ids)
        slot_in, slot_out = self.plan.assign(ids, restarted)
        if n == 0:
            return None
        if max(n, int(alive)) > self.capacity:
            self._grow(max(n, int(alive), 2 * self.capacity))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        s01 = s01.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(t)
        prev = self._in
        if self.motion is not None:
            nb = -(-self.S // self.motion.block)
            self.last_vectors = torch.empty((n, nb, nb, 2), dtype=torch.int32, device=self.device)
            prev = self._warp
        for b0 in range(0, n, photo.MAX_BATCH):
            b1 = min(n, b0 + photo.MAX_BATCH)
            if self.motion is not None:
                motion_warp(s01[b0:b1], self._in[0], self._in[1], slot_in[b0:b1], prev[0], prev[1], self.motion, self.last_vectors[b0:b1])
                self.motion_launches += 1
            temporal_diff(t[b0:b1], s01[b0:b1], prev[0], prev[1], slot_in[b0:b1], self._out[0], self._out[1], slot_out[b0:b1], self.filt,
                          out=out[b0:b1])
            self.launches += 1
        self._in, self._out = self._out, self._in
        return out


# ---- the session --------------------------------------------------------------------------------------------------------------------
FrameRecord = namedtuple('FrameRecord', 'tracks restarted raw regions decoded src01 filtered')
FrameRecord.__doc__ = """What a push did with one frame (VideoSession.last): the track id of every face in the detector's order, whether
the track (re)started here, the regions as found and as cropped and pasted (smoothed), and the face rows [n,3,S,S] of the decoded
samples, of the crops the model saw and of the samples the paste got (``filtered`` is ``decoded`` without a temporal filter); the three
tensors are None for a frame without a face."""


class VideoSession:
    """TestDiffuseModel.video_session: one clip, fed in pushes of any length.  See there."""

    def __init__(self, model, ref_photo, ref_box=None, seed=None, size: int = 256, feather: int = 8, max_faces: int = 4, face_batch: int = 8,
                 align: bool = False, min_roll: float = 5.0, guided_paste=None, temporal=TemporalFilter(), box_smooth: float = 0.5,
                 tracker: Optional[FaceTracker] = None, own_pixels: bool = False, batch: Optional[dict] = None,
                 motion: Optional[MotionSearch] = None, teacher_start=None):
        from .face_parser import find_faces
        if teacher_start is not None or getattr(model, 'teacher_start', None) is not None:
            raise ValueError('teacher_start is not combined with video sessions (video_session / transfer_video)')
        if own_pixels:
            raise ValueError('video_session: own_pixels is not combined with video (a track has no owner map across frames)')
        if not isinstance(ref_photo, torch.Tensor) or ref_photo.dim() != 3:
            raise ValueError('video_session: ONE reference photo (a uint8 [H,W,3] tensor) serves every track; per-track references are not supported')
        if temporal is not None and not isinstance(temporal, TemporalFilter):
            raise ValueError(f'video_session: temporal must be a video.TemporalFilter or None, got {temporal!r}')
        if motion is not None and not isinstance(motion, MotionSearch):
            raise ValueError(f'video_session: motion must be a video.MotionSearch or None, got {motion!r}')
        if motion is not None and temporal is None:
            raise ValueError('video_session: motion compensates the temporal filter: it needs temporal (a video.TemporalFilter), got temporal=None')
        if guided_paste is not None and not isinstance(guided_paste, photo.GuidedPaste):
            raise ValueError(f'guided_paste must be a photo.GuidedPaste or None, got {guided_paste!r}')
        if tracker is not None and not isinstance(tracker, FaceTracker):
            raise ValueError(f'video_session: tracker must be a video.FaceTracker or None, got {tracker!r}')
        K, fb = int(max_faces), int(face_batch)
        if K != max_faces or not 1 <= K <= 64:
            raise ValueError(f'max_faces must be an integer 1..64, got {max_faces!r}')
        if fb != face_batch or fb < 1:
            raise ValueError(f'face_batch must be an integer >= 1, got {face_batch!r}')
        if align and not float(min_roll) >= 0.0:
            raise ValueError(f'min_roll must be >= 0 degrees, got {min_roll!r}')
        self.gamma = check_box_smooth(box_smooth)
        self.size, self.feather = photo._check_size(size), photo._check_feather(feather)
        self.model, self.K, self.fb, self.align, self.guided, self.temporal = model, K, fb, bool(align), guided_paste, temporal
        model._check_unipc_masked()
        if not model.has_first_stage:
            raise ValueError('video_session pastes decoded images: it needs a first stage (first_stage_config)')
        if seed is None:
            seed = model.seed
        if seed is not None:
            from .noise import as_seeds
            seed = as_seeds(seed, 1).seeds[0]
        self.seed = seed
        # the text of the clip: ONE row of the fields get_input reads (txt_emb / txt_tokens / txt), used by every face; None: 'makeup transfer'
        self.text = None if batch is None else {k: v for k, v in batch.items() if k in ('txt_emb', 'txt_tokens', model.cond_stage_key)}
        for k, v in ({} if self.text is None else self.text).items():
            if len(v) != 1:
                raise ValueError(f'video_session: batch[{k!r}] must hold ONE row, the text of the clip, got {len(v)}')
        self.look = dict(parse_size=model.parse_size, lut=model.parser_lut)
        if self.align:
            self.look.update(oriented=True, min_roll=float(min_roll))
        self.eng = model._require_engine()
        self.ref = ref_photo.to(model.device)
        if ref_box is None:
            if model.face_parser is None:
                raise ValueError('video_session: ref_box is needed (only an attached face parser can find the reference face)')
            found = find_faces(model.face_parser, [self.ref], max_faces=1, **self.look)[0]
            if not found:
                raise ValueError('video_session: the reference photo shows no face')
            self.ref_region = found[0]
        else:
            self.ref_region = self._region(ref_box)
        self.tracker = tracker if tracker is not None else FaceTracker()
        self.state = None if temporal is None else TemporalState(temporal, self.size, model.device, capacity=K, motion=motion)
        self._hat: Dict[int, object] = {}          # alive tracks: id -> the smoothed region of the track's last frame
        self.frames_seen = 0
        self.chunks: List[Tuple[int, int]] = []          # the last push: (items, batch it was sampled at) per chunk
        self.last: List[FrameRecord] = []

    def _region(self, b):          # (x0, y0, w, h[, angle]) or a Frame -> the box itself when it is upright, else its Frame
        if isinstance(b, photo.Frame):
            return b
        if len(b) == 4 or (self.align and len(b) == 5 and float(b[4]) == 0.0):
            return tuple(int(v) for v in b[:4])
        if self.align and len(b) == 5:
            return photo.frame_from_box(b[:4], float(b[4]))
        raise ValueError(f'a box is (x0, y0, w, h){" or (x0, y0, w, h, angle)" if self.align else ""}, got {b!r}')

    def _track(self, found) -> Tuple[List[int], List[bool], list]:
        """the host decisions of one frame: ids, restart flags and the smoothed regions of its faces"""
        ids = self.tracker.update(found)
        restarted = list(self.tracker.restarted)
        regions = []
        for tid, fresh, raw in zip(ids, restarted, found):
            reg = smooth_frame(None if fresh else self._hat.get(tid), raw, self.gamma)
            self._hat[tid] = reg
            regions.append(reg)
        for tid in [k for k in self._hat if k not in ids]:          # a track that missed a frame starts its smoothing over
            del self._hat[tid]
        return ids, restarted, regions

    @torch.no_grad()
    def push(self, frames, src_boxes=None, src_segs=None):
        """the next frames of the clip (a list of uint8 [H,W,3] tensors) -> the made-up frames, as clones on the device.
        ``src_boxes``: one LIST of boxes per frame (None: the attached parser finds the faces); ``src_segs``: one label map per frame
        at the frame's resolution, for fix_background / paste_background."""
        from .face_parser import find_faces
        from .noise import Seeds
        m, eng = self.model, self.eng
        frames = photo.as_list(frames, 3)
        F = len(frames)
        if src_boxes is None and m.face_parser is None:
            raise ValueError('video: src_boxes are needed (only an attached face parser can find the faces)')
        if src_boxes is not None:
            src_boxes = list(src_boxes)
            if len(src_boxes) != F:
                raise ValueError(f'video: src_boxes must hold one LIST of boxes per frame ({F}), got {len(src_boxes)} entries')
            for i, bl in enumerate(src_boxes):
                if len(bl) > self.K:
                    raise ValueError(f'video: src_boxes[{i}] holds {len(bl)} boxes, more than max_faces = {self.K}')
        if src_segs is not None and len(src_segs) != F:
            raise ValueError(f'{F} frames but {len(src_segs)} label maps')
        if (m.fix_background or m.paste_background) and src_segs is None and m.face_parser is None:
            raise KeyError('video: fix_background / paste_background need src_segs (label maps at the frames\' resolution)')
        frames = [p.to(m.device) for p in frames]
        if not F:
            self.last = []
            return []
        # 1. the faces of every pushed frame
        if src_boxes is None:
            found = [[self._region(b) for b in fl] for fl in find_faces(m.face_parser, frames, max_faces=self.K, **self.look)]
        else:
            found = [[self._region(b) for b in bl] for bl in src_boxes]
        # 2. tracks and crops, frame by frame on the host
        tracked = [self._track(fl) for fl in found]
        alive_after = len(self.tracker.alive)
        # 3. every (frame, face) of the push through the single photo pass, in chunks
        items = [(f, k) for f in range(F) for k in range(len(found[f]))]
        phi = float(m.guidance_rescale)
        imgs, srcs = [], []
        self.chunks = []
        for c0 in range(0, len(items), self.fb):
            chunk = items[c0:c0 + self.fb]
            real = len(chunk)
            # With a seed every chunk runs at the SAME batch, face_batch: a ragged chunk is filled up with repeats of its last item
            # and their rows are dropped.  The GEMM planner picks tiles by shape, so only then do the decoded images -- like the
            # tracks and the noise -- not depend on how the clip is split into pushes.  A seeded draw has no generator state, so
            # the repeats change nothing else; without a seed they would move the torch generators, and the chunk stays as it is
            # (the transfer_photos calls)
            if self.seed is not None:
                chunk = chunk + [chunk[-1]] * (self.fb - real)
            self.chunks.append((real, len(chunk)))
            pick = [f for f, _ in chunk]
            extra, text = {}, None
            if self.text is not None:
                text = {k: (v.expand(len(chunk), *v.shape[1:]).contiguous() if isinstance(v, torch.Tensor) else [v[0]] * len(chunk))
                        for k, v in self.text.items()}
            if self.seed is not None:          # 4. the clip's seed, the track as the sub-stream
                extra['seeds'] = Seeds((self.seed,) * len(chunk), tuple(tracked[f][0][k] for f, k in chunk))
            img, src = m._photo_pass([frames[f] for f in pick], [self.ref] * len(chunk), [tracked[f][2][k] for f, k in chunk],
                                     [self.ref_region] * len(chunk), None if src_segs is None else [src_segs[f] for f in pick], None, self.size,
                                     text, phi, **extra)
            imgs.append(img[:real])
            srcs.append(src[:real])
        out = [p.clone(memory_format=torch.contiguous_format) for p in frames]
        self.frames_seen += F
        if not items:
            if self.state is not None:
                for _ in range(F):
                    self.state.step([], None, None)
            self.last = [FrameRecord(*tr[:2], found[f], tr[2], None, None, None) for f, tr in enumerate(tracked)]
            return out
        img, src = torch.cat(imgs), torch.cat(srcs)
        # 5. the temporal filter, frame by frame in order: one launch over the faces of a frame (it depends on the previous frame's
        # state only; no paste reads it, so all of them come before the pastes)
        rows = img
        if self.state is not None:
            rows = img.clone()
            j = 0
            for f in range(F):
                n = len(found[f])
                if n:
                    rows[j:j + n] = self.state.step(tracked[f][0], img[j:j + n], src[j:j + n], tracked[f][1], alive=alive_after)
                else:
                    self.state.step([], None, None)
                j += n
        # ... and the pastes as transfer_photos makes them: rank by rank, largest first, a frame once per launch
        for rank in range(max(len(fl) for fl in found)):
            sel = [j for j, (_, k) in enumerate(items) if k == rank]
            at = torch.tensor(sel, device=img.device)
            eng.paste_regions([out[items[j][0]] for j in sel], [tracked[items[j][0]][2][rank] for j in sel], rows[at], src[at], self.feather, None,
                              self.guided)
        self.last, j = [], 0
        for f, tr in enumerate(tracked):
            n = len(found[f])
            part = (lambda x: x[j:j + n]) if n else (lambda x: None)
            self.last.append(FrameRecord(tr[0], tr[1], found[f], tr[2], part(img), part(src), part(rows)))
            j += n
        return out


def transfer_video(model, frames, ref_photo, frame_batch: int = 8, src_boxes=None, src_segs=None, **session_kwargs):
    """TestDiffuseModel.transfer_video: one session fed ``frame_batch`` frames at a time -> the made-up frames"""
    fbatch = int(frame_batch)
    if fbatch != frame_batch or fbatch < 1:
        raise ValueError(f'frame_batch must be an integer >= 1, got {frame_batch!r}')
    frames = photo.as_list(frames, 3)
    for name, v in (('src_boxes', src_boxes), ('src_segs', src_segs)):
        if v is not None and len(v) != len(frames):
            raise ValueError(f'{len(frames)} frames but {len(v)} entries of {name}')
    session = VideoSession(model, ref_photo, **session_kwargs)
    out = []
    for f0 in range(0, len(frames), fbatch):
        part = lambda v: None if v is None else list(v[f0:f0 + fbatch])
        out += session.push(frames[f0:f0 + fbatch], part(src_boxes), part(src_segs))
    return out
