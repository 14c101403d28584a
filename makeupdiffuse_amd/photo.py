"""Full-resolution photos on the device: any-size uint8 photo + face box -> the model's src_img / ref_img / label map
(mkd_crop_resize: the bytes of Pillow's antialiased bilinear ``Image.resize((S, S), Image.BILINEAR, box=...)``), and the decoded
sample back into the photo at its own resolution with the photo's fine detail kept (mkd_paste_photo, build-defined after the
Laplacian detail transfer of PSGAN / EleGANt ``Inference.postprocess``).  include/mkd.h states both rules.

Photos are uint8 [H,W,3] device tensors (rows may be ``pitch`` bytes apart: stride (pitch, 3, 1), any alignment); the photos of one
call may differ in size.  Boxes are (x0, y0, w, h) in photo pixels.  The arithmetic is libmkd's: there is no CPU path."""
from __future__ import annotations

import ctypes as C
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


def _photo_list(photos, what: str) -> List[torch.Tensor]:
    if isinstance(photos, torch.Tensor):
        photos = [photos] if photos.dim() == 3 else list(photos.unbind(0))
    photos = list(photos)
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


def _descs(photos: Sequence[torch.Tensor], boxes, labels: Optional[Sequence[torch.Tensor]]):
    arr = (_lib.PhotoDescC * len(photos))()
    for i, (p, (x0, y0, bw, bh)) in enumerate(zip(photos, boxes)):
        H, W = int(p.shape[0]), int(p.shape[1])
        arr[i].pixels = p.data_ptr()
        arr[i].pitch_bytes = int(p.stride(0)) if H > 1 else 3 * W
        arr[i].H, arr[i].W = H, W
        arr[i].x0, arr[i].y0, arr[i].bw, arr[i].bh = x0, y0, bw, bh
        arr[i].labels = None if labels is None else labels[i].data_ptr()
    return arr


def crop_resize(photos, boxes, size: int, labels=None, want_u8: bool = False) -> Cropped:
    """photos (a list of uint8 [H,W,3] device tensors, or one [B,H,W,3] tensor) and their boxes (x0, y0, w, h) ->
    Cropped(img01 fp32 [B,3,S,S] = float(u8) / 255 of Pillow's antialiased bilinear resize of the box to S x S (the values
    PairFolderDataset._load gives for that crop), labels uint8 [B,S,S] or None, u8 uint8 [B,S,S,3] or None).  ``labels``: one uint8
    [H,W] label map per photo at the photo's resolution, sampled at the output pixel centres without interpolation."""
    S = _check_size(size)
    photos = _photo_list(photos, 'crop_resize')
    B = len(photos)
    if len(boxes) != B:
        raise ValueError(f'{B} photos but {len(boxes)} boxes')
    boxes = [check_box(b, int(p.shape[0]), int(p.shape[1]), S) for p, b in zip(photos, boxes)]
    dev = photos[0].device
    photos = [p if _rows_ok(p) else p.contiguous() for p in photos]
    if labels is not None:
        if isinstance(labels, torch.Tensor):
            labels = [labels] if labels.dim() == 2 else list(labels.unbind(0))
        labels = list(labels)
        if len(labels) != B:
            raise ValueError(f'{B} photos but {len(labels)} label maps')
        lab = []
        for p, l in zip(photos, labels):
            if not isinstance(l, torch.Tensor) or l.dtype != torch.uint8 or tuple(l.shape) != tuple(p.shape[:2]):
                raise ValueError(f'a label map is a uint8 [H,W] tensor of its photo\'s size {tuple(p.shape[:2])}, '
                                 f'got {getattr(l, "dtype", type(l))} {tuple(getattr(l, "shape", ()))}')
            lab.append(l.to(dev).contiguous())
        labels = lab
    lib = _lib.load()
    img01 = torch.empty((B, 3, S, S), device=dev, dtype=torch.float32)
    lab_out = torch.empty((B, S, S), device=dev, dtype=torch.uint8) if labels is not None else None
    u8 = torch.empty((B, S, S, 3), device=dev, dtype=torch.uint8) if want_u8 else None
    P = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    with torch.cuda.device(dev):
        for b0 in range(0, B, MAX_BATCH):
            b1 = min(B, b0 + MAX_BATCH)
            arr = _descs(photos[b0:b1], boxes[b0:b1], None if labels is None else labels[b0:b1])
            nbytes = int(lib.mkd_crop_resize_scratch_bytes(arr, b1 - b0, S))
            if nbytes <= 0:
                raise _lib.MkdError('mkd_crop_resize_scratch_bytes refused the descriptors')
            scratch = torch.empty((nbytes + 256,), device=dev, dtype=torch.uint8)       # (the stream keeps it alive until the kernels ran)
            base = (scratch.data_ptr() + 255) & ~255
            _lib.check(lib.mkd_crop_resize(arr, b1 - b0, S, P(img01[b0:b1]), P(None if u8 is None else u8[b0:b1]),
                                           P(None if lab_out is None else lab_out[b0:b1]), C.c_void_p(base), C.c_void_p(_stream())),
                       'mkd_crop_resize')
    return Cropped(img01, lab_out, u8)


def paste_photos(photos, boxes, samples: torch.Tensor, src01: torch.Tensor, feather: int = 8, weights: Optional[torch.Tensor] = None):
    """The decoded ``samples`` (fp32 [B,3,S,S], nominally [-1, 1]) back into ``photos`` IN PLACE, inside their boxes only:
    photo + a * upsampled((samples + 1) / 2 - src01) * 255, rounded to uint8 (ties to even), where src01 is the img01 the model saw
    (crop_resize of the same photos and boxes) and a fades from 1 / (feather + 1) at a box side to 1 over ``feather`` photo pixels
    (sides on the photo's border do not fade).  Only the difference is interpolated, so everything finer than the model's grid stays
    the photo's own.  ``weights`` (fp32 [B,wh,ww], wh, ww <= 2048; mkd_paste_photo_weighted): plane b covers the WHOLE of photo b at
    low resolution and a is multiplied by its bilinear sample at the photo pixel (components.owner_weights: each face's paste stays
    on its own pixels); a weight of 0 leaves the photo's byte.  Returns ``photos``."""
    rho = int(feather)
    if rho != feather or not 0 <= rho <= MAX_FEATHER:
        raise ValueError(f'feather must be an integer 0..{MAX_FEATHER} photo pixels, got {feather!r}')
    plist = _photo_list(photos, 'paste_photos')
    B = len(plist)
    if len(boxes) != B:
        raise ValueError(f'{B} photos but {len(boxes)} boxes')
    if samples.dim() != 4 or samples.shape[0] != B or samples.shape[1] != 3 or samples.shape[2] != samples.shape[3]:
        raise ValueError(f'samples must be [{B},3,S,S], got {tuple(samples.shape)}')
    if tuple(src01.shape) != tuple(samples.shape):
        raise ValueError(f'src01 {tuple(src01.shape)} must have the shape of samples {tuple(samples.shape)}')
    S = _check_size(int(samples.shape[2]))
    boxes = [check_box(b, int(p.shape[0]), int(p.shape[1]), S) for p, b in zip(plist, boxes)]
    for p in plist:
        if not _rows_ok(p):
            raise ValueError('paste_photos writes in place: a photo needs interleaved RGB rows (stride (pitch, 3, 1))')
    dev = plist[0].device
    t = samples.to(device=dev, dtype=torch.float32).contiguous()
    s = src01.to(device=dev, dtype=torch.float32).contiguous()
    w = None
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dim() != 3 or weights.shape[0] != B or weights.dtype != torch.float32 \
                or not (1 <= weights.shape[1] <= MAX_WEIGHT_SIDE and 1 <= weights.shape[2] <= MAX_WEIGHT_SIDE):
            raise ValueError(f'weights must be fp32 [{B},wh,ww] with wh, ww in 1..{MAX_WEIGHT_SIDE}, got '
                             f'{getattr(weights, "dtype", type(weights))} {tuple(getattr(weights, "shape", ()))}')
        w = weights.to(device=dev).contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        for b0 in range(0, B, MAX_BATCH):
            b1 = min(B, b0 + MAX_BATCH)
            arr = _descs(plist[b0:b1], boxes[b0:b1], None)
            if w is None:
                _lib.check(lib.mkd_paste_photo(arr, b1 - b0, S, C.c_void_p(t[b0:b1].data_ptr()), C.c_void_p(s[b0:b1].data_ptr()), rho,
                                               C.c_void_p(_stream())), 'mkd_paste_photo')
            else:
                _lib.check(lib.mkd_paste_photo_weighted(arr, b1 - b0, S, C.c_void_p(t[b0:b1].data_ptr()), C.c_void_p(s[b0:b1].data_ptr()), rho,
                                                        C.c_void_p(w[b0:b1].data_ptr()), int(w.shape[1]), int(w.shape[2]), C.c_void_p(_stream())),
                           'mkd_paste_photo_weighted')
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
    if isinstance(labels, torch.Tensor):
        labels = [labels] if labels.dim() == 2 else list(labels.unbind(0))
    out = []
    for l in labels:
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
    blank lines and lines starting with # are skipped."""
    out: Dict[str, List[Tuple[int, int, int, int]]] = {}
    with open(path, 'r') as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 5:
                raise ValueError(f'{path}:{ln}: expected "name x0 y0 w h", got {line.strip()!r}')
            try:
                out.setdefault(parts[0], []).append(tuple(int(v) for v in parts[1:]))
            except ValueError:
                raise ValueError(f'{path}:{ln}: the box of {parts[0]} must hold four integers') from None
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
        x0, y0, bw, bh = box
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
        return torch.from_numpy(a), tuple(int(v) for v in box), seg

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
