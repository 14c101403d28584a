"""Connected components of a label map on the device (include/mkd.h mkd_label_components): the 8-connected sets of the pixels whose
label is in a class set, with id (smallest linear index), area and inclusive bounding box each, the largest ``max_out`` as a table.
What face_parser.find_faces builds on: one component of the face classes is one face.  owner_map (mkd_owner_map) then gives every
pixel the table component nearest to it and owner_weights (mkd_owner_weights) each component's share of a pixel's neighbourhood:
what keeps one face's paste off its neighbour; face_frames (mkd_face_frames) measures every component's roll from its two eye classes
and its extent in its own frame: what photo.grow_frame turns into an oriented crop.  Integer arithmetic only (one division per weight), so the outputs are exact and the
same bytes on every run.  The arithmetic is libmkd's: there is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import lib as _lib

MAX_OUT = 64
MAX_PIXELS = 1 << 24
ROW = 6                                          # id, area, r0, r1, c0, c1
FILL_ROW = (-1, 0, 2 ** 31 - 1, -1, 2 ** 31 - 1, -1)          # a table row past the last component (the library's empty box)


def class_bits(classes: Sequence[int]) -> int:
    """the bit set of mkd_region_mask_from_labels: bit l = label l"""
    bits = 0
    for c in classes:
        if int(c) != c or not 0 <= int(c) < 64:
            raise ValueError(f'a class must be an integer label 0..63, got {c!r}')
        bits |= 1 << int(c)
    return bits


def label_components(labels: torch.Tensor, classes: Sequence[int], min_area: int = 1, max_out: int = 16,
                     want_ids: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """labels uint8 [B,H,W] or [H,W] on the device -> (table int32 [B,max_out,6], count int32 [B], ids int32 [B,H,W] or None), device
    tensors.  Components are the 8-connected sets of the pixels whose label is in ``classes``; a table row is (id, area, row min, row
    max, col min, col max) with id the component's smallest linear index y * W + x.  count[b] is the number of components with area >=
    min_area (not capped); the table holds the largest max_out of them, area descending, ties by id ascending, then FILL_ROW rows.
    ids (want_ids) carries the id at every pixel of ANY component, also the ones below min_area, and -1 elsewhere.  Nothing is
    read back: the call only enqueues (four launches)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() not in (2, 3):
        raise ValueError(f'labels must be uint8 [B,H,W] or [H,W], got {getattr(labels, "dtype", type(labels))} {tuple(getattr(labels, "shape", ()))}')
    if labels.device.type != 'cuda':
        raise _lib.MkdError('label_components: labels must be on a HIP device (there is no CPU implementation)')
    if int(max_out) != max_out or not 1 <= int(max_out) <= MAX_OUT:
        raise ValueError(f'max_out must be an integer 1..{MAX_OUT}, got {max_out!r}')
    if int(min_area) != min_area or int(min_area) < 1:
        raise ValueError(f'min_area must be an integer >= 1, got {min_area!r}')
    bits = class_bits(classes)
    lab = (labels[None] if labels.dim() == 2 else labels).contiguous()
    B, H, W = (int(v) for v in lab.shape)
    if B < 1 or H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f'labels {tuple(lab.shape)}: B, H, W >= 1 and H * W <= 2^24')
    dev = lab.device
    lib = _lib.load()
    table = torch.empty((B, int(max_out), ROW), device=dev, dtype=torch.int32)
    count = torch.empty((B,), device=dev, dtype=torch.int32)
    ids = torch.empty((B, H, W), device=dev, dtype=torch.int32) if want_ids else None
    nbytes = int(lib.mkd_label_components_scratch_bytes(B, H, W))
    if nbytes <= 0:
        raise _lib.MkdError('mkd_label_components_scratch_bytes refused the shape')
    scratch = torch.empty((nbytes + 256,), device=dev, dtype=torch.uint8)          # (the stream keeps it alive until the kernels ran)
    base = (scratch.data_ptr() + 255) & ~255
    with torch.cuda.device(dev):
        _lib.check(lib.mkd_label_components(C.c_void_p(lab.data_ptr()), B, H, W, C.c_uint64(bits), int(min_area), int(max_out),
                                            C.c_void_p(table.data_ptr()), C.c_void_p(count.data_ptr()),
                                            C.c_void_p(None if ids is None else ids.data_ptr()), C.c_void_p(base),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mkd_label_components')
    return table, count, ids


NO_OWNER = 255                                   # owner of every pixel of an image without seeds
NO_DIST = 2 ** 31 - 1
MAX_SIDE = 2048                                  # mkd_owner_map / mkd_owner_weights: H, W
MAX_ITEMS = 16                                   # (image, rank) planes per mkd_owner_weights call; more are split here
MAX_OWNER_FEATHER = 16


def owner_map(ids: torch.Tensor, table: torch.Tensor, want_dist: bool = False):
    """ids int32 [B,H,W] and table int32 [B,max_out,6] of ONE label_components call (device tensors) -> owner uint8 [B,H,W]: the rank
    (table row) of the component nearest to every pixel in the exact Euclidean metric of the ids' own grid, ties to the lower rank;
    NO_OWNER in an image whose table is empty.  Only components IN the table are seeds.  want_dist: (owner, dist2 int32 [B,H,W]), the
    squared distance (NO_DIST without seeds).  Nothing is read back: the call only enqueues (two launches)."""
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 3:
        raise ValueError(f'ids must be int32 [B,H,W], got {getattr(ids, "dtype", type(ids))} {tuple(getattr(ids, "shape", ()))}')
    B, H, W = (int(v) for v in ids.shape)
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 3 or table.shape[0] != B or table.shape[2] != ROW \
            or not 1 <= table.shape[1] <= MAX_OUT:
        raise ValueError(f'table must be int32 [{B},1..{MAX_OUT},{ROW}], got {getattr(table, "dtype", type(table))} {tuple(getattr(table, "shape", ()))}')
    if ids.device.type != 'cuda' or table.device != ids.device:
        raise _lib.MkdError('owner_map: ids and table must be on one HIP device (there is no CPU implementation)')
    if B < 1 or not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f'ids {tuple(ids.shape)}: B >= 1 and H, W in 1..{MAX_SIDE}')
    ids, table = ids.contiguous(), table.contiguous()
    dev = ids.device
    lib = _lib.load()
    owner = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
    dist = torch.empty((B, H, W), device=dev, dtype=torch.int32) if want_dist else None
    nbytes = int(lib.mkd_owner_map_scratch_bytes(B, H, W))
    if nbytes <= 0:
        raise _lib.MkdError('mkd_owner_map_scratch_bytes refused the shape')
    scratch = torch.empty((nbytes + 256,), device=dev, dtype=torch.uint8)          # (the stream keeps it alive until the kernels ran)
    base = (scratch.data_ptr() + 255) & ~255
    with torch.cuda.device(dev):
        _lib.check(lib.mkd_owner_map(C.c_void_p(ids.data_ptr()), C.c_void_p(table.data_ptr()), B, H, W, int(table.shape[1]),
                                     C.c_void_p(owner.data_ptr()), C.c_void_p(None if dist is None else dist.data_ptr()), C.c_void_p(base),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mkd_owner_map')
    return (owner, dist) if want_dist else owner


def owner_weights(owner: torch.Tensor, items: Sequence[Tuple[int, int]], feather: int = 2) -> torch.Tensor:
    """owner uint8 [B,H,W] (owner_map) and items [(image, rank), ...] -> fp32 [len(items),H,W]: per item the fraction of the
    (2 feather + 1)^2 window around every pixel (indices clamped to the edge) that image's rank owns; feather 0 is the 0 / 1
    indicator.  One launch per MAX_ITEMS items; nothing is read back."""
    if not isinstance(owner, torch.Tensor) or owner.dtype != torch.uint8 or owner.dim() != 3:
        raise ValueError(f'owner must be uint8 [B,H,W], got {getattr(owner, "dtype", type(owner))} {tuple(getattr(owner, "shape", ()))}')
    if owner.device.type != 'cuda':
        raise _lib.MkdError('owner_weights: owner must be on a HIP device (there is no CPU implementation)')
    rho = int(feather)
    if rho != feather or not 0 <= rho <= MAX_OWNER_FEATHER:
        raise ValueError(f'feather must be an integer 0..{MAX_OWNER_FEATHER}, got {feather!r}')
    B, H, W = (int(v) for v in owner.shape)
    items = [(int(i), int(r)) for i, r in items]
    if not items:
        raise ValueError('owner_weights: no items')
    for i, r in items:
        if not 0 <= i < B or not 0 <= r < MAX_OUT:
            raise ValueError(f'item {(i, r)}: the image must lie in 0..{B - 1} and the rank in 0..{MAX_OUT - 1}')
    owner = owner.contiguous()
    dev = owner.device
    lib = _lib.load()
    out = torch.empty((len(items), H, W), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        for n0 in range(0, len(items), MAX_ITEMS):
            part = items[n0:n0 + MAX_ITEMS]
            flat = (C.c_int32 * (2 * len(part)))(*[v for it in part for v in it])
            _lib.check(lib.mkd_owner_weights(C.c_void_p(owner.data_ptr()), B, H, W, flat, len(part), rho, C.c_void_p(out[n0:].data_ptr()),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mkd_owner_weights')
    return out


FRAME_UNIT = 16384                               # |(cq, sq)| of a face frame
FRAME_ROW = 8                                    # n_a, n_b, cq, sq, umin, umax, vmin, vmax
MAX_FRAME_BATCH = 16                             # images per mkd_face_frames call (photo sizes travel by value); more are split here
MAX_FRAME_SIDE = 4096


def face_frames(labels: torch.Tensor, ids: torch.Tensor, table: torch.Tensor, photo_hw, classes_a: Sequence[int] = (4,),
                classes_b: Sequence[int] = (5,), min_eye_area: Optional[int] = None) -> torch.Tensor:
    """Every face's roll and its extent in its own frame (mkd_face_frames).  labels uint8 and ids int32 [B,S,S] on the square squashed
    grid of face_parser.find_faces, ids and table int32 [B,max_out,6] of ONE label_components call, photo_hw [(H, W), ...] the size of
    the photo behind every image -> int64 [B,max_out,8] on the device, a row (n_a, n_b, cq, sq, umin, umax, vmin, vmax): the pixels of
    the component in ``classes_a`` / ``classes_b`` (LUT_SEG's two eyes), the direction from the centroid of a to that of b in PHOTO
    pixels as integers of length FRAME_UNIT ((FRAME_UNIT, 0): upright; also when an eye has fewer than ``min_eye_area`` pixels --
    default max(1, (S // 128)^2) -- or the roll exceeds 60 degrees), and the component's extent along and across that direction in
    units of 1 / (2 S FRAME_UNIT) photo pixel (photo.grow_frame turns a row into a crop).  Integers: the same bytes on every run.
    Nothing is read back: the call only enqueues (four launches per MAX_FRAME_BATCH images)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3 or labels.shape[1] != labels.shape[2]:
        raise ValueError(f'labels must be uint8 [B,S,S], got {getattr(labels, "dtype", type(labels))} {tuple(getattr(labels, "shape", ()))}')
    B, S = int(labels.shape[0]), int(labels.shape[1])
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or tuple(ids.shape) != (B, S, S):
        raise ValueError(f'ids must be int32 [{B},{S},{S}], got {getattr(ids, "dtype", type(ids))} {tuple(getattr(ids, "shape", ()))}')
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 3 or table.shape[0] != B or table.shape[2] != ROW \
            or not 1 <= table.shape[1] <= MAX_OUT:
        raise ValueError(f'table must be int32 [{B},1..{MAX_OUT},{ROW}], got {getattr(table, "dtype", type(table))} {tuple(getattr(table, "shape", ()))}')
    if labels.device.type != 'cuda' or ids.device != labels.device or table.device != labels.device:
        raise _lib.MkdError('face_frames: labels, ids and table must be on one HIP device (there is no CPU implementation)')
    if B < 1 or not 1 <= S <= MAX_FRAME_SIDE:
        raise ValueError(f'labels {tuple(labels.shape)}: B >= 1 and S in 1..{MAX_FRAME_SIDE}')
    hw = [(int(h), int(w)) for h, w in photo_hw]
    if len(hw) != B or any(not (1 <= h <= 16384 and 1 <= w <= 16384) for h, w in hw):
        raise ValueError(f'photo_hw must hold {B} pairs (H, W) in 1..16384, got {photo_hw!r}')
    area = max(1, (S // 128) ** 2) if min_eye_area is None else int(min_eye_area)
    if area < 1 or (min_eye_area is not None and area != min_eye_area):
        raise ValueError(f'min_eye_area must be an integer >= 1, got {min_eye_area!r}')
    bits_a, bits_b = class_bits(classes_a), class_bits(classes_b)
    labels, ids, table = labels.contiguous(), ids.contiguous(), table.contiguous()
    K = int(table.shape[1])
    dev = labels.device
    lib = _lib.load()
    raw = torch.empty((B, K, 6), device=dev, dtype=torch.int64)          # mkd_face_frame: 48 bytes, four int32 then four int64
    with torch.cuda.device(dev):
        for b0 in range(0, B, MAX_FRAME_BATCH):
            n = min(B, b0 + MAX_FRAME_BATCH) - b0
            nbytes = int(lib.mkd_face_frames_scratch_bytes(n, K))
            if nbytes <= 0:
                raise _lib.MkdError('mkd_face_frames_scratch_bytes refused the shape')
            scratch = torch.empty((nbytes + 256,), device=dev, dtype=torch.uint8)          # (the stream keeps it alive until the kernels ran)
            base = (scratch.data_ptr() + 255) & ~255
            flat = (C.c_int32 * (2 * n))(*[v for pair in hw[b0:b0 + n] for v in pair])
            _lib.check(lib.mkd_face_frames(C.c_void_p(labels[b0:].data_ptr()), C.c_void_p(ids[b0:].data_ptr()), C.c_void_p(table[b0:].data_ptr()),
                                           n, S, K, flat, C.c_uint64(bits_a), C.c_uint64(bits_b), area, C.c_void_p(raw[b0:].data_ptr()),
                                           C.c_void_p(base), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mkd_face_frames')
    head = raw.view(torch.int32).reshape(B, K, 12)[..., :4].to(torch.int64)
    return torch.cat((head, raw[..., 2:]), 2)
