"""Connected components of a label map on the device (include/mkd.h mkd_label_components): the 8-connected sets of the pixels whose
label is in a class set, with id (smallest linear index), area and inclusive bounding box each, the largest ``max_out`` as a table.
What face_parser.find_faces builds on: one component of the face classes is one face.  Integer arithmetic only, so the outputs are
exact and the same bytes on every run.  The arithmetic is libmkd's: there is no CPU path."""
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
