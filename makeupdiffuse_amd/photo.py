"""Full-resolution photos on the device: any-size uint8 photo + face box -> the model's src_img / ref_img / label map
(mkd_crop_resize: the bytes of Pillow's antialiased bilinear ``Image.resize((S, S), Image.BILINEAR, box=...)``), and the decoded
sample back into the photo at its own resolution with the photo's fine detail kept (mkd_paste_photo, build-defined after the
Laplacian detail transfer of PSGAN / EleGANt ``Inference.postprocess``).  include/mkd.h states both rules.

Photos are uint8 [H,W,3] device tensors (rows may be ``pitch`` bytes apart: stride (pitch, 3, 1), any alignment); the photos of one
call may differ in size.  Boxes are (x0, y0, w, h) in photo pixels.  Tilted faces take the same path along a rotated square, a Frame
(cx, cy, side, c, s): crop_frames / paste_frames (mkd_crop_frame, mkd_paste_frame), and crop_regions / paste_regions for batches that
mix boxes and frames.  The arithmetic is libmkd's: there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import namedtuple
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _lib

MAX_BATCH = 16          # descriptors per library call (MKD_PHOTO_MAX_BATCH); larger batches are split here
MAX_FEATHER = 64
MIN_SIZE, MAX_SIZE = 8, 1024
MAX_SIDE = 16384
MAX_WEIGHT_SIDE = 2048  # rows / columns of a paste's photo-wide weight plane
# the reference's crop around a detected face (diffdata/preprocessing.py:18): fractions of the face box added above, below and per side
UP_RATIO, DOWN_RATIO, WIDTH_RATIO = 0.6 / 0.85, 0.2 / 0.85, 0.2 / 0.85

Cropped = namedtuple('Cropped', 'img01 labels u8')
# an oriented square: centre and side in photo pixels (pixel (X, Y) has its centre at (X + .5, Y + .5)), (c, s) the unit vector of the
# face's "right" axis; (-s, c) is its "down" axis and c = 1, s = 0 is upright (include/mkd.h mkd_photo_frame_desc)
Frame = namedtuple('Frame', 'cx cy side c s')
GUIDE_RADII = (0, 1, 2)
GUIDE_SIGMA_MIN, GUIDE_SIGMA_MAX = 0.5, 1e6


class GuidedPaste(namedtuple('GuidedPaste', 'radius sigma')):
    """Edge-aware paste (include/mkd.h mkd_paste_photo_guided / mkd_paste_frame_guided): the makeup difference is brought up to the
    photo by joint bilateral upsampling under the photo's own luminance instead of bilinearly, so it stops at the photo's edges.
    ``radius`` 0, 1 or 2: the taps reach radius + 1 model pixels per side; ``sigma``: the luminance distance, in 8-bit levels
    (0.5 .. 1e6), at which a tap's weight has fallen to a half."""
    __slots__ = ()

    def __new__(cls, radius: int = 1, sigma: float = 8.0):
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or int(radius) not in GUIDE_RADII:
            raise ValueError(f'GuidedPaste: radius must be 0, 1 or 2, got {radius!r}')
        try:
            sg = float(sigma)
        except (TypeError, ValueError):
            sg = math.nan
        if not (math.isfinite(sg) and GUIDE_SIGMA_MIN <= sg <= GUIDE_SIGMA_MAX):
            raise ValueError(f'GuidedPaste: sigma must be a finite number of luminance levels in [{GUIDE_SIGMA_MIN}, {GUIDE_SIGMA_MAX:g}], got {sigma!r}')
        return super().__new__(cls, int(radius), sg)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def resize_ksize(length: int, size: int) -> int:
    """taps per output index of one axis: 2 ceil(max(length / size, 1)) + 1"""
    return 2 * max(1, -(-int(length) // int(size))) + 1


def check_box(box, H: int, W: int, size: int) -> Tuple[int, int, int, int]:
    """(x0, y0, w, h) as ints, validated against the photo and the library's limits (include/mkd.h mkd_photo_desc)"""
    if len(box) != 4:
        raise ValueError(f'a box is (x0, y0, w, h), got {box!r}')
    x0, y0, bw, bh = (int(v) for v in box)
    if any(int(v) != v for v in box):
        raise ValueError(f'box {box!r} must hold integers')
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f'photo {H}x{W}: H, W must be 1..{MAX_SIDE}')
    if bw < 1 or bh < 1 or x0 < 0 or y0 < 0 or x0 + bw > W or y0 + bh > H:
        raise ValueError(f'box {(x0, y0, bw, bh)} is empty or not inside the {H}x{W} photo')
    if bw > 32 * size or bh > 32 * size:
        raise ValueError(f'box {(x0, y0, bw, bh)} exceeds 32 x size = {32 * size} per side')
    return x0, y0, bw, bh


def _check_size(size: int) -> int:
    if int(size) != size or not MIN_SIZE <= int(size) <= MAX_SIZE:
        raise ValueError(f'size must be an integer {MIN_SIZE}..{MAX_SIZE}, got {size!r}')
    return int(size)


def as_list(ts, rank: int) -> list:
    """one tensor of ``rank`` dimensions, a stacked batch of such tensors (``rank`` + 1 dimensions) or a sequence of them -> a list"""
    if isinstance(ts, torch.Tensor):
        return [ts] if ts.dim() == rank else list(ts.unbind(0))
    return list(ts)


def _photo_list(photos, what: str) -> List[torch.Tensor]:
    photos = as_list(photos, 3)
    if not photos:
        raise ValueError(f'{what}: no photos')
    for p in photos:
        if not isinstance(p, torch.Tensor) or p.dtype != torch.uint8 or p.dim() != 3 or p.shape[2] != 3:
            raise ValueError(f'{what}: a photo is a uint8 [H,W,3] tensor, got {getattr(p, "dtype", type(p))} {tuple(getattr(p, "shape", ()))}')
        if p.device.type != 'cuda':
            raise _lib.MkdError(f'{what}: photos must be on a HIP device (there is no CPU implementation)')
    return photos


def _rows_ok(p: torch.Tensor) -> bool:
    """interleaved RGB rows a fixed number of bytes apart: what a descriptor can address as it is"""
    return p.stride(2) == 1 and p.stride(1) == 3 and (p.shape[0] == 1 or p.stride(0) >= 3 * p.shape[1])


# ---- tilted faces: the same path along a rotated square (include/mkd.h mkd_crop_frame, mkd_paste_frame; this build's rule) ----------
def frame_from_box(box, angle_deg: float = 0.0) -> Frame:
    """the square box (x0, y0, w, h) rotated about its centre by ``angle_deg`` (the face's "right" axis turns from +x towards +y,
    which points DOWN in a photo) as a Frame.  Multiples of 90 degrees give exact 0 / +-1 for c and s.  A Frame is a square: a
    non-square box raises ValueError (with angle 0 such a box needs no Frame: crop_resize takes it as it is)."""
    if len(box) != 4:
        raise ValueError(f'a box is (x0, y0, w, h), got {box!r}')
    x0, y0, bw, bh = (float(v) for v in box)
    a = float(angle_deg)
    if not (bw > 0 and bh > 0) or not math.isfinite(a):
        raise ValueError(f'box {box!r} / angle {angle_deg!r}: the box must be non-empty and the angle finite')
    if bw != bh:
        raise ValueError(f'box {box!r} is not square: only a square box can be rotated into a Frame (angle {angle_deg!r})')
    quarter = a / 90.0
    if quarter == int(quarter):
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter) % 4]
    else:
        c, s = math.cos(math.radians(a)), math.sin(math.radians(a))
    return Frame(x0 + bw / 2.0, y0 + bh / 2.0, bw, c, s)


def box_from_frame(frame) -> Optional[Tuple[int, int, int, int]]:
    """the integer box (x0, y0, side, side) an UPRIGHT frame (c = 1, s = 0) with integer corners stands for, else None: such a frame
    takes crop_resize / paste_photos, the calls of the axis-aligned path"""
    f = Frame(*frame)
    if f.s != 0 or f.c != 1:
        return None
    x0, y0 = f.cx - f.side / 2.0, f.cy - f.side / 2.0
    if x0 != int(x0) or y0 != int(y0) or f.side != int(f.side) or f.side < 1:
        return None
    return int(x0), int(y0), int(f.side), int(f.side)


def frame_roll(row) -> float:
    """degrees of roll of a components.face_frames row (n_a, n_b, cq, sq, ...)"""
    return math.degrees(math.atan2(int(row[3]), int(row[2])))


def grow_frame(face_frame_row, S: int, H: int, W: int, grow: float = 1.0) -> Frame:
    """A components.face_frames row (n_a, n_b, cq, sq, umin, umax, vmin, vmax) of a face found on the S x S squashed map of an H x W
    photo -> the crop around it as a Frame.  (1) the extents become photo pixels along the unit axes e_u = (cq, sq) / |(cq, sq)| and
    e_v = (-sq, cq) / |(cq, sq)|: divided by 2 S |(cq, sq)| (= 2 S 16384 up to the rounding of cq and sq), and widened by half the
    footprint of a squashed pixel, (|c| W / S + |s| H / S) / 2 along e_u and (|s| W / S + |c| H / S) / 2 along e_v (the extents are those
    of pixel CENTRES; find_faces scales its boxes outwards in the same way); (2) grow_square_box's ratios IN THAT FRAME: up 0.6/0.85 and
    down 0.2/0.85 of the height along e_v, 0.2/0.85 of the width per side along e_u, times ``grow``; (3) squared about its centre with
    the longer side, the side limited to min(H, W); (4) the centre rotated back to photo coordinates.  The frame is NOT shifted into
    the photo: the crop replicates edges and the paste writes only what lies inside."""
    row = [int(v) for v in face_frame_row]
    if len(row) != 8:
        raise ValueError(f'a face frame row holds 8 integers (n_a, n_b, cq, sq, umin, umax, vmin, vmax), got {face_frame_row!r}')
    _, _, cq, sq, umin, umax, vmin, vmax = row
    if umax < umin or vmax < vmin:
        raise ValueError('the face frame row is empty (a table row past the last component): there is no frame to grow')
    if not grow >= 0:
        raise ValueError(f'grow must be >= 0, got {grow!r}')
    norm = math.hypot(cq, sq)
    if norm == 0:
        raise ValueError(f'the face frame row has no direction: (cq, sq) = {(cq, sq)}')
    c, s = cq / norm, sq / norm
    unit = 2.0 * S * norm
    pad_u = (abs(c) * W / S + abs(s) * H / S) / 2.0
    pad_v = (abs(s) * W / S + abs(c) * H / S) / 2.0
    u0, u1 = umin / unit - pad_u, umax / unit + pad_u
    v0, v1 = vmin / unit - pad_v, vmax / unit + pad_v
    fw, fh = u1 - u0, v1 - v0
    top, bottom = v0 - grow * UP_RATIO * fh, v1 + grow * DOWN_RATIO * fh
    left, right = u0 - grow * WIDTH_RATIO * fw, u1 + grow * WIDTH_RATIO * fw
    side = float(min(max(bottom - top, right - left), H, W))
    uc, vc = (left + right) / 2.0, (top + bottom) / 2.0
    return Frame(c * uc - s * vc, s * uc + c * vc, side, c, s)


def check_frame(frame, H: int, W: int, size: int) -> Frame:
    """a Frame of floats, validated against the photo and the library's limits (include/mkd.h mkd_photo_frame_desc)"""
    if len(frame) != 5:
        raise ValueError(f'a frame is (cx, cy, side, c, s), got {frame!r}')
    f = Frame(*(float(v) for v in frame))
    if not all(math.isfinite(v) for v in f):
        raise ValueError(f'frame {frame!r} must hold finite numbers')
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f'photo {H}x{W}: H, W must be 1..{MAX_SIDE}')
    if not 0 < f.side <= 32 * size:
        raise ValueError(f'frame {tuple(f)}: the side must lie in (0, 32 x size = {32 * size}]')
    if abs(f.c * f.c + f.s * f.s - 1.0) > 1e-9:
        raise ValueError(f'frame {tuple(f)}: (c, s) must be a unit vector')
    if not (-f.side <= f.cx <= W + f.side and -f.side <= f.cy <= H + f.side):
        raise ValueError(f'frame {tuple(f)}: the centre must lie within one side of the {H}x{W} photo')
    return f


# ---- one crop and one paste for both kinds of region ---------------------------------------------------------------------------------
def _label_list(labels, photos, dev) -> Optional[List[torch.Tensor]]:
    if labels is None:
        return None
    labels = as_list(labels, 2)
    if len(labels) != len(photos):
        raise ValueError(f'{len(photos)} photos but {len(labels)} label maps')
    out = []
    for p, l in zip(photos, labels):
        if not isinstance(l, torch.Tensor) or l.dtype != torch.uint8 or tuple(l.shape) != tuple(p.shape[:2]):
            raise ValueError(f'a label map is a uint8 [H,W] tensor of its photo\'s size {tuple(p.shape[:2])}, '
                             f'got {getattr(l, "dtype", type(l))} {tuple(getattr(l, "shape", ()))}')
        out.append(l.to(dev).contiguous())
    return out


def _check_feather(feather) -> int:
    rho = int(feather)
    if rho != feather or not 0 <= rho <= MAX_FEATHER:
        raise ValueError(f'feather must be an integer 0..{MAX_FEATHER} photo pixels, got {feather!r}')
    return rho


def _check_paste(what: str, plist, regions, samples, src01, weights) -> int:
    B = len(plist)
    if len(regions) != B:
        raise ValueError(f'{B} photos but {len(regions)} {what}')
    if samples.dim() != 4 or samples.shape[0] != B or samples.shape[1] != 3 or samples.shape[2] != samples.shape[3]:
        raise ValueError(f'samples must be [{B},3,S,S], got {tuple(samples.shape)}')
    if tuple(src01.shape) != tuple(samples.shape):
        raise ValueError(f'src01 {tuple(src01.shape)} must have the shape of samples {tuple(samples.shape)}')
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dim() != 3 or weights.shape[0] != B or weights.dtype != torch.float32 \
                or not (1 <= weights.shape[1] <= MAX_WEIGHT_SIDE and 1 <= weights.shape[2] <= MAX_WEIGHT_SIDE):
            raise ValueError(f'weights must be fp32 [{B},wh,ww] with wh, ww in 1..{MAX_WEIGHT_SIDE}, got '
                             f'{getattr(weights, "dtype", type(weights))} {tuple(getattr(weights, "shape", ()))}')
    return _check_size(int(samples.shape[2]))


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(None if t is None else t.data_ptr())


# The library calls of the two kinds on one chunk of at most MAX_BATCH descriptors: a crop into (img01, u8, labels), each a tensor or
# None, and a paste of (t, s01) weighted by w (a tensor or None).
def _crop_box(lib, arr, n, S, img01, u8, lab_out):
    nbytes = int(lib.mkd_crop_resize_scratch_bytes(arr, n, S))
    if nbytes <= 0:
        raise _lib.MkdError('mkd_crop_resize_scratch_bytes refused the descriptors')
    scratch = torch.empty((nbytes + 256,), device=img01.device, dtype=torch.uint8)       # (the stream keeps it alive until the kernels ran)
    base = (scratch.data_ptr() + 255) & ~255
    _lib.check(lib.mkd_crop_resize(arr, n, S, _ptr(img01), _ptr(u8), _ptr(lab_out), C.c_void_p(base), C.c_void_p(_stream())), 'mkd_crop_resize')


def _crop_frame(lib, arr, n, S, img01, u8, lab_out):
    _lib.check(lib.mkd_crop_frame(arr, n, S, _ptr(img01), _ptr(u8), _ptr(lab_out), C.c_void_p(_stream())), 'mkd_crop_frame')


def _plane(w):
    return (_ptr(w), 0, 0) if w is None else (_ptr(w), int(w.shape[1]), int(w.shape[2]))


def _paste_box(lib, arr, n, S, t, s, rho, w, guided):
    if guided is not None:
        _lib.check(lib.mkd_paste_photo_guided(arr, n, S, _ptr(t), _ptr(s), rho, *_plane(w), guided.radius, guided.sigma, C.c_void_p(_stream())),
                   'mkd_paste_photo_guided')
    elif w is None:
        _lib.check(lib.mkd_paste_photo(arr, n, S, _ptr(t), _ptr(s), rho, C.c_void_p(_stream())), 'mkd_paste_photo')
    else:
        _lib.check(lib.mkd_paste_photo_weighted(arr, n, S, _ptr(t), _ptr(s), rho, _ptr(w), int(w.shape[1]), int(w.shape[2]), C.c_void_p(_stream())),
                   'mkd_paste_photo_weighted')


def _paste_frame(lib, arr, n, S, t, s, rho, w, guided):
    if guided is not None:
        _lib.check(lib.mkd_paste_frame_guided(arr, n, S, _ptr(t), _ptr(s), rho, *_plane(w), guided.radius, guided.sigma, C.c_void_p(_stream())),
                   'mkd_paste_frame_guided')
    else:
        _lib.check(lib.mkd_paste_frame(arr, n, S, _ptr(t), _ptr(s), rho, *_plane(w), C.c_void_p(_stream())), 'mkd_paste_frame')


def _fill_box(d, box):
    d.x0, d.y0, d.bw, d.bh = box


def _fill_frame(d, frame):
    d.cx, d.cy, d.side, d.c, d.s = frame


# a kind of region: what messages call its entries, its checker, its descriptor type and what writes a checked region into one, and
# its crop and paste: the name of the public entry and the library call
_Kind = namedtuple('_Kind', 'noun check desc fill crop_name crop paste_name paste')
_BOX = _Kind('boxes', check_box, _lib.PhotoDescC, _fill_box, 'crop_resize', _crop_box, 'paste_photos', _paste_box)
_FRAME = _Kind('frames', check_frame, _lib.PhotoFrameDescC, _fill_frame, 'crop_frames', _crop_frame, 'paste_frames', _paste_frame)


def _descs(kind: _Kind, photos: Sequence[torch.Tensor], regions, labels: Optional[Sequence[torch.Tensor]]):
    arr = (kind.desc * len(photos))()          # (zeroed: labels stays null without a label map)
    for i, (d, p, r) in enumerate(zip(arr, photos, regions)):
        H, W = p.shape[0], p.shape[1]
        d.pixels = p.data_ptr()
        d.pitch_bytes = p.stride(0) if H > 1 else 3 * W
        d.H, d.W = H, W
        if labels is not None:
            d.labels = labels[i].data_ptr()
        kind.fill(d, r)
    return arr


def _crop(kind: _Kind, photos, regions, size: int, labels, want_u8: bool) -> Cropped:
    S = _check_size(size)
    photos = _photo_list(photos, kind.crop_name)
    B = len(photos)
    if len(regions) != B:
        raise ValueError(f'{B} photos but {len(regions)} {kind.noun}')
    regions = [kind.check(r, int(p.shape[0]), int(p.shape[1]), S) for p, r in zip(photos, regions)]
    dev = photos[0].device
    photos = [p if _rows_ok(p) else p.contiguous() for p in photos]
    labels = _label_list(labels, photos, dev)
    lib = _lib.load()
    img01 = torch.empty((B, 3, S, S), device=dev, dtype=torch.float32)
    lab_out = torch.empty((B, S, S), device=dev, dtype=torch.uint8) if labels is not None else None
    u8 = torch.empty((B, S, S, 3), device=dev, dtype=torch.uint8) if want_u8 else None
    part = lambda t, b0, b1: None if t is None else t[b0:b1]
    with torch.cuda.device(dev):
        for b0 in range(0, B, MAX_BATCH):
            b1 = min(B, b0 + MAX_BATCH)
            kind.crop(lib, _descs(kind, photos[b0:b1], regions[b0:b1], part(labels, b0, b1)), b1 - b0, S, img01[b0:b1], part(u8, b0, b1),
                      part(lab_out, b0, b1))
    return Cropped(img01, lab_out, u8)


def _check_guided(guided) -> Optional[GuidedPaste]:
    if guided is not None and not isinstance(guided, GuidedPaste):
        raise ValueError(f'guided must be a photo.GuidedPaste or None, got {guided!r}')
    return guided


def _paste(kind: _Kind, photos, regions, samples: torch.Tensor, src01: torch.Tensor, feather: int, weights: Optional[torch.Tensor],
           guided: Optional[GuidedPaste] = None):
    # one order of checks for both kinds: feather, guided, photos, counts and shapes, weights, size, regions, rows.  Against the two copies
    # this replaces, paste_frames now looks at the feather before the photos, and paste_photos at the weights before the boxes and rows
    rho = _check_feather(feather)
    guided = _check_guided(guided)
    plist = _photo_list(photos, kind.paste_name)
    S = _check_paste(kind.noun, plist, regions, samples, src01, weights)
    B = len(plist)
    regions = [kind.check(r, int(p.shape[0]), int(p.shape[1]), S) for p, r in zip(plist, regions)]
    for p in plist:
        if not _rows_ok(p):
            raise ValueError(f'{kind.paste_name} writes in place: a photo needs interleaved RGB rows (stride (pitch, 3, 1))')
    dev = plist[0].device
    t = samples.to(device=dev, dtype=torch.float32).contiguous()
    s = src01.to(device=dev, dtype=torch.float32).contiguous()
    w = None if weights is None else weights.to(device=dev).contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        for b0 in range(0, B, MAX_BATCH):
            b1 = min(B, b0 + MAX_BATCH)
            kind.paste(lib, _descs(kind, plist[b0:b1], regions[b0:b1], None), b1 - b0, S, t[b0:b1], s[b0:b1], rho, None if w is None else w[b0:b1],
                       guided)
    return photos


def crop_resize(photos, boxes, size: int, labels=None, want_u8: bool = False) -> Cropped:
    """photos (a list of uint8 [H,W,3] device tensors, or one [B,H,W,3] tensor) and their boxes (x0, y0, w, h) ->
    Cropped(img01 fp32 [B,3,S,S] = float(u8) / 255 of Pillow's antialiased bilinear resize of the box to S x S (the values
    PairFolderDataset._load gives for that crop), labels uint8 [B,S,S] or None, u8 uint8 [B,S,S,3] or None).  ``labels``: one uint8
    [H,W] label map per photo at the photo's resolution, sampled at the output pixel centres without interpolation."""
    return _crop(_BOX, photos, boxes, size, labels, want_u8)


def paste_photos(photos, boxes, samples: torch.Tensor, src01: torch.Tensor, feather: int = 8, weights: Optional[torch.Tensor] = None,
                 guided: Optional[GuidedPaste] = None):
    """The decoded ``samples`` (fp32 [B,3,S,S], nominally [-1, 1]) back into ``photos`` IN PLACE, inside their boxes only:
    photo + a * upsampled((samples + 1) / 2 - src01) * 255, rounded to uint8 (ties to even), where src01 is the img01 the model saw
    (crop_resize of the same photos and boxes) and a fades from 1 / (feather + 1) at a box side to 1 over ``feather`` photo pixels
    (sides on the photo's border do not fade).  Only the difference is interpolated, so everything finer than the model's grid stays
    the photo's own.  ``weights`` (fp32 [B,wh,ww], wh, ww <= 2048; mkd_paste_photo_weighted): plane b covers the WHOLE of photo b at
    low resolution and a is multiplied by its bilinear sample at the photo pixel (components.owner_weights: each face's paste stays
    on its own pixels); a weight of 0 leaves the photo's byte.  ``guided`` (a GuidedPaste; mkd_paste_photo_guided): the difference is
    upsampled under the photo's own luminance edges instead of bilinearly; None makes exactly the calls above.  Returns ``photos``."""
    return _paste(_BOX, photos, boxes, samples, src01, feather, weights, guided)


def crop_frames(photos, frames, size: int, labels=None, want_u8: bool = False) -> Cropped:
    """crop_resize along ROTATED squares (mkd_crop_frame): photos and their Frames (cx, cy, side, c, s) -> Cropped(img01 fp32
    [B,3,S,S], labels uint8 [B,S,S] or None, u8 uint8 [B,S,S,3] or None).  The face's "right" axis (c, s) becomes the crop's +x: a
    rolled face comes out upright.  Pillow's triangle filter taken in the face's frame, in double and in one pass (within 1 of
    crop_resize's bytes for an upright integer box); the square may stick out of the photo, edges are replicated; labels are
    sampled at the output pixel centres without interpolation."""
    return _crop(_FRAME, photos, frames, size, labels, want_u8)


def paste_frames(photos, frames, samples: torch.Tensor, src01: torch.Tensor, feather: int = 8, weights: Optional[torch.Tensor] = None,
                 guided: Optional[GuidedPaste] = None):
    """paste_photos along ROTATED squares (mkd_paste_frame), IN PLACE: every photo pixel whose centre lies in its Frame gets
    photo + a * g * bilinear((samples + 1) / 2 - src01) * 255 sampled at its place in the frame, in double; a fades over ``feather``
    photo pixels at ALL four sides of the square, g is the bilinear sample of ``weights`` (fp32 [B,wh,ww] over the whole photo, as in
    paste_photos) or 1.  Bytes outside the square, and everything of a square that does not reach its photo, stay.  ``guided`` as in
    paste_photos (mkd_paste_frame_guided).  Returns ``photos``."""
    return _paste(_FRAME, photos, frames, samples, src01, feather, weights, guided)


def split_regions(regions):
    """regions (boxes (x0, y0, w, h) and Frames, mixed) -> (indices that take the axis-aligned calls, their boxes, indices that take
    the frame calls, their Frames): a box, and a Frame that box_from_frame can turn into one, go the axis-aligned way"""
    bi, boxes, fi, frames = [], [], [], []
    for i, r in enumerate(regions):
        box = tuple(r) if len(r) == 4 else box_from_frame(r)
        if box is not None:
            bi.append(i)
            boxes.append(box)
        else:
            fi.append(i)
            frames.append(Frame(*r))
    return bi, boxes, fi, frames


def crop_regions(photos, regions, size: int, labels=None) -> Cropped:
    """crop_resize for boxes and crop_frames for rolled Frames in one batch, results in the order of ``regions``.  Without a rolled
    Frame this is exactly ONE crop_resize call on the whole batch."""
    photos = _photo_list(photos, 'crop_regions')
    if len(regions) != len(photos):
        raise ValueError(f'{len(photos)} photos but {len(regions)} regions')
    bi, boxes, fi, frames = split_regions(regions)
    if not fi:
        return crop_resize(photos, boxes, size, labels=labels)
    labels = _label_list(labels, photos, photos[0].device)
    pick = lambda seq, idx: None if seq is None else [seq[i] for i in idx]
    cf = crop_frames(pick(photos, fi), frames, size, labels=pick(labels, fi))
    if not bi:
        return cf
    cb = crop_resize(pick(photos, bi), boxes, size, labels=pick(labels, bi))
    order = torch.tensor(bi + fi, device=cf.img01.device).argsort()
    merge = lambda a, b: None if a is None else torch.cat((a, b))[order]
    return Cropped(merge(cb.img01, cf.img01), merge(cb.labels, cf.labels), None)


def paste_regions(photos, regions, samples: torch.Tensor, src01: torch.Tensor, feather: int = 8, weights: Optional[torch.Tensor] = None,
                  guided: Optional[GuidedPaste] = None):
    """paste_photos for boxes and paste_frames for rolled Frames in one batch (a photo appears once per call, so the split changes
    nothing).  Without a rolled Frame this is exactly ONE paste_photos call on the whole batch.  ``guided`` goes to both."""
    _check_guided(guided)
    plist = _photo_list(photos, 'paste_regions')
    if len(regions) != len(plist):
        raise ValueError(f'{len(plist)} photos but {len(regions)} regions')
    bi, boxes, fi, frames = split_regions(regions)
    if not fi:
        paste_photos(plist, boxes, samples, src01, feather, weights, guided)
        return photos
    for idx, regs, fn in ((bi, boxes, paste_photos), (fi, frames, paste_frames)):
        if idx:
            at = torch.tensor(idx, device=samples.device)
            fn([plist[i] for i in idx], regs, samples[at], src01[at], feather, None if weights is None else weights[at.to(weights.device)],
               guided)
    return photos


def resize_coeffs(n: int, in0: int, length: int, size: int, device=None):
    """The coefficient table of one axis as the device builds it (mkd_resize_coeffs; debugging and tests): (bounds int32 [S,2] =
    (xmin, xmax), coefficients int32 [S, ksize])."""
    S = _check_size(size)
    dev = torch.device('cuda' if device is None else device)
    bounds = torch.empty((S, 2), device=dev, dtype=torch.int32)
    coef = torch.empty((S, resize_ksize(length, S)), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mkd_resize_coeffs(int(n), int(in0), int(length), S, C.c_void_p(bounds.data_ptr()), C.c_void_p(coef.data_ptr()),
                                                 C.c_void_p(_stream())), 'mkd_resize_coeffs')
    return bounds, coef


def grow_square_box(box, H: int, W: int, grow: float = 1.0) -> Tuple[int, int, int, int]:
    """(row min, row max, col min, col max) of a face, inclusive -> the square crop (x0, y0, side, side) around it: the face box grown
    by ``grow`` times the reference's ratios (up 0.6/0.85 and down 0.2/0.85 of its height, 0.2/0.85 of its width per side), made
    square about its centre with the longer side, limited to the photo's shorter side and shifted inside the photo."""
    r0, r1, c0, c1 = (int(v) for v in box)
    if r1 < r0 or c1 < c0:
        raise ValueError('the label map holds no pixel of the face classes: there is no box to grow')
    if not grow >= 0:
        raise ValueError(f'grow must be >= 0, got {grow!r}')
    fh, fw = r1 - r0 + 1, c1 - c0 + 1
    top, bottom = r0 - grow * UP_RATIO * fh, r1 + 1 + grow * DOWN_RATIO * fh
    left, right = c0 - grow * WIDTH_RATIO * fw, c1 + 1 + grow * WIDTH_RATIO * fw
    side = min(int(round(max(bottom - top, right - left))), H, W)
    x0 = int(round((left + right - side) / 2.0))
    y0 = int(round((top + bottom - side) / 2.0))
    x0 = min(max(x0, 0), W - side)
    y0 = min(max(y0, 0), H - side)
    return x0, y0, side, side


def square_box_from_labels(labels, classes: Iterable[int] = (1, 2, 3, 4, 5, 6, 7, 9, 11), grow: float = 1.0) -> List[Tuple[int, int, int, int]]:
    """Face boxes from label maps at photo resolution (one uint8 [H,W] device tensor, a list of them, or [B,H,W]): the bounding box
    of ``classes`` that mkd_region_mask_from_labels returns, grown and squared by grow_square_box.  Reads the boxes back (one small
    device-to-host copy per photo size): set-up, not the hot path."""
    from . import makeup_score as ms
    out = []
    for l in as_list(labels, 2):
        if l.dim() != 2:
            raise ValueError(f'a label map is [H,W], got {tuple(l.shape)}')
        _, _, box = ms.region_mask(l[None], classes, box_classes=classes, margin=0)
        out.append(grow_square_box(box[0].tolist(), int(l.shape[0]), int(l.shape[1]), grow))
    return out


def centred_square(H: int, W: int) -> Tuple[int, int, int, int]:
    """the centred largest square of an H x W photo"""
    side = min(H, W)
    return (W - side) // 2, (H - side) // 2, side, side


def read_boxes_multi(path: str) -> Dict[str, List[Tuple[int, int, int, int]]]:
    """Lines of '<image name> x0 y0 w h' -> {name: [(x0, y0, w, h), ...]}: a name may repeat, one line per face, kept in file order;
    blank lines and lines starting with # are skipped.  A line may carry a sixth field, the face's roll in degrees ('<image name> x0
    y0 w h angle'): it reads as the 5-tuple (x0, y0, w, h, angle) that transfer_photos(align=True) takes."""
    out: Dict[str, List[Tuple[int, int, int, int]]] = {}
    with open(path, 'r') as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) not in (5, 6):
                raise ValueError(f'{path}:{ln}: expected "name x0 y0 w h" or "name x0 y0 w h angle", got {line.strip()!r}')
            try:
                box = tuple(int(v) for v in parts[1:5])
            except ValueError:
                raise ValueError(f'{path}:{ln}: the box of {parts[0]} must hold four integers') from None
            if len(parts) == 6:
                try:
                    angle = float(parts[5])
                except ValueError:
                    angle = math.nan
                if not math.isfinite(angle):
                    raise ValueError(f'{path}:{ln}: the angle of {parts[0]} must be a finite number of degrees') from None
                box = box + (angle,)
            out.setdefault(parts[0], []).append(box)
    return out


def read_boxes(path: str) -> Dict[str, Tuple[int, int, int, int]]:
    """Lines of '<image name> x0 y0 w h' -> {name: (x0, y0, w, h)}; blank lines and lines starting with # are skipped.  Of a name
    that repeats (a multi-face file, read_boxes_multi) the FIRST line counts."""
    return {name: boxes[0] for name, boxes in read_boxes_multi(path).items()}


class PhotoPairDataset:
    """root/images/<name> + a pairs file at the photos' NATIVE resolution: dicts with src_photo / ref_photo (uint8 [H,W,3]), src_box /
    ref_box (x0, y0, w, h) from root/boxes.txt ('name x0 y0 w h' per line) or else the centred largest square, txt and img_name as
    PairFolderDataset gives them, and src_seg / ref_seg (uint8 [H,W] at photo resolution) when root/scgan_segs/ exists."""

    def __init__(self, root: str, pairs_file: str = 'test_0412.txt', boxes_file: str = 'boxes.txt', prompt: str = 'makeup transfer'):
        from .imageio import read_pairs
        self.root = root
        self.pairs = read_pairs(pairs_file if os.path.isabs(pairs_file) else os.path.join(root, pairs_file))
        bp = boxes_file if os.path.isabs(boxes_file) else os.path.join(root, boxes_file)
        self.faces = read_boxes_multi(bp) if os.path.exists(bp) else {}          # every line of a name (multi-face files)
        self.boxes = {name: boxes[0] for name, boxes in self.faces.items()}
        self.prompt = prompt
        self.has_segs = os.path.isdir(os.path.join(root, 'scgan_segs'))

    def __len__(self) -> int:
        return len(self.pairs)

    def _load(self, name: str):
        from PIL import Image
        a = np.array(Image.open(os.path.join(self.root, 'images', name)).convert('RGB'), dtype=np.uint8)
        H, W = a.shape[:2]
        box = self.boxes.get(name, centred_square(H, W))
        x0, y0, bw, bh = box[:4]
        if bw < 1 or bh < 1 or x0 < 0 or y0 < 0 or x0 + bw > W or y0 + bh > H:
            raise ValueError(f'box {box} of {name} is empty or not inside the {H}x{W} photo')
        seg = None
        if self.has_segs:
            s = Image.open(os.path.join(self.root, 'scgan_segs', name))
            if s.mode not in ('L', 'P'):
                s = s.convert('L')
            if s.size != (W, H):
                raise ValueError(f'label map of {name} is {s.size[1]}x{s.size[0]}, the photo {H}x{W}: label maps are at photo resolution')
            seg = torch.from_numpy(np.array(s, dtype=np.uint8))
        return torch.from_numpy(a), tuple(int(v) for v in box[:4]), seg          # (a line's angle stays in self.faces)

    def __getitem__(self, i: int) -> Dict[str, object]:
        s, r = self.pairs[i]
        (sp, sb, ss), (rp, rb, rs) = self._load(s), self._load(r)
        base = lambda n: os.path.basename(n).split('.')[0]
        out = {'src_photo': sp, 'ref_photo': rp, 'src_box': sb, 'ref_box': rb, 'txt': self.prompt, 'img_name': f'{base(s)}&{base(r)}'}
        if self.has_segs:
            out['src_seg'], out['ref_seg'] = ss, rs
        return out


def collate_photos(items: Sequence[Dict[str, object]]) -> Dict[str, list]:
    """photos of a batch differ in size: every field becomes a list"""
    return {k: [it[k] for it in items] for k in items[0]}
