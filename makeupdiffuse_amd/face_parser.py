"""The face-parsing network on the device: label maps from images (include/mkd.h mkd_parser_*).

UPSTREAM: zllrunning/face-parsing.PyTorch (BiSeNet with a ResNet-18 context path) as vendored by PSGAN / EleGANt ``faceutils/mask``;
the reference runs it in its preprocessing (diffdata/preprocessing.py:38,151-157): parse at 512 x 512, nearest resize of the label map,
class remap.  State-dict names are upstream's; they are unverified against a real checkpoint file (none was at hand).  The arithmetic
is libmkd's: there is no CPU path.

Two remap tables over upstream's 19 CelebAMask-HQ classes (bg, skin, l_brow, r_brow, l_eye, r_eye, eye_g, l_ear, r_ear, ear_r, nose,
mouth, u_lip, l_lip, neck, neck_l, cloth, hair, hat):
LUT_PREPROCESS is the reference's own class list (preprocessing.py:53-54); LUT_SEG is the convention every consumer in this
repository uses (skin 1, nose 6, neck 13: diffmk/makeups.py:179-199; teeth 11, hair 12: the Fixbackground classes; lips 7 / 9).  In
LUT_SEG both ears go to 8, a label no class set here selects: that choice is this build's."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _lib

CLASS_NAMES = ('bg', 'skin', 'l_brow', 'r_brow', 'l_eye', 'r_eye', 'eye_g', 'l_ear', 'r_ear', 'ear_r', 'nose', 'mouth', 'u_lip', 'l_lip',
               'neck', 'neck_l', 'cloth', 'hair', 'hat')
LUT_PREPROCESS = (0, 1, 2, 3, 4, 5, 0, 11, 12, 0, 6, 8, 7, 9, 13, 0, 0, 10, 0)
LUT_SEG = (0, 1, 2, 3, 4, 5, 0, 8, 8, 0, 6, 11, 7, 9, 13, 0, 0, 12, 0)
FACE_CLASSES = (1, 2, 3, 4, 5, 6, 7, 9, 11)          # LUT_SEG labels that make up the face box (photo.square_box_from_labels' default)
MIN_SIZE, MAX_SIZE, MAX_BATCH = 64, 1024, 64


@dataclass
class FaceParserConfig:
    n_classes: int = 19
    widths: Tuple[int, int, int, int] = (64, 128, 256, 512)
    blocks: Tuple[int, int, int, int] = (2, 2, 2, 2)
    cp_channels: int = 128
    ffm_channels: int = 256
    bn_eps: float = 1e-5
    mean: Tuple[float, float, float] = (0.485, 0.456, 0.406)
    std: Tuple[float, float, float] = (0.229, 0.224, 0.225)

    def to_c(self) -> _lib.ParserConfigC:
        c = _lib.ParserConfigC()
        c.n_classes, c.cp_channels, c.ffm_channels, c.bn_eps = int(self.n_classes), int(self.cp_channels), int(self.ffm_channels), float(self.bn_eps)
        for i in range(4):
            c.widths[i], c.blocks[i] = int(self.widths[i]), int(self.blocks[i])
        for i in range(3):
            c.mean[i], c.std[i] = float(self.mean[i]), float(self.std[i])
        return c


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _check_lut(lut, n_classes: int):
    if lut is None:
        return None
    lut = [int(v) for v in lut]
    if len(lut) != n_classes or any(not 0 <= v <= 255 for v in lut):
        raise ValueError(f'lut must hold {n_classes} values in 0..255, got {lut!r}')
    return (C.c_uint8 * n_classes)(*lut)


def parse_labels(logits: torch.Tensor, parse_size: Tuple[int, int], out_size: Optional[Tuple[int, int]] = None, lut=None) -> torch.Tensor:
    """The head alone (mkd_parse_labels): fp32 logits [B,C,h8,w8] of any strides (NCHW, or an NHWC tensor permuted) -> labels uint8
    [B,out_h,out_w]: bilinear (align_corners=True) to ``parse_size``, the reference's nearest resize to ``out_size``, argmax (first
    maximum), ``lut``."""
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise ValueError(f'logits must be fp32 [B,C,h,w], got {logits.dtype} {tuple(logits.shape)}')
    if logits.device.type != 'cuda':
        raise _lib.MkdError('parse_labels: logits must be on a HIP device (there is no CPU implementation)')
    B, nc, h8, w8 = (int(v) for v in logits.shape)
    P_h, P_w = (int(v) for v in parse_size)
    out_h, out_w = (P_h, P_w) if out_size is None else (int(v) for v in out_size)
    labels = torch.empty((B, max(out_h, 0), max(out_w, 0)), device=logits.device, dtype=torch.uint8)
    sb, sc, sr, sx = (int(v) for v in logits.stride())
    with torch.cuda.device(logits.device):
        _lib.check(_lib.load().mkd_parse_labels(C.c_void_p(logits.data_ptr()), sc, sr, sx, sb, B, nc, h8, w8, P_h, P_w, out_h, out_w,
                                                _check_lut(lut, nc), C.c_void_p(labels.data_ptr()), C.c_void_p(_stream())), 'mkd_parse_labels')
    return labels


class FaceParser:
    """BiSeNet face parsing on the device.  ``FaceParser(cfg).load(path)`` (or ``load_state_dict`` / ``init_random``), ``finalize()``,
    then ``parse(img01)``: RGB images in [0, 1], fp32 [B,3,H,W] with H and W multiples of 32 in 64..1024 -> uint8 label maps."""

    def __init__(self, cfg: Optional[FaceParserConfig] = None, device=None):
        self.cfg = cfg or FaceParserConfig()
        self.device = torch.device('cuda' if device is None else device)
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.mkd_parser_create(C.byref(self.cfg.to_c()), C.byref(h)), 'mkd_parser_create')          # host only
        self._h = h
        self.finalized = False

    # ---- weights ------------------------------------------------------------------------------------------
    def expected_params(self) -> Dict[str, Tuple[int, ...]]:
        """{state-dict name: shape}, sorted by name (host only)"""
        out = {}
        shp = (C.c_int64 * 4)()
        for i in range(self.lib.mkd_parser_param_total(self._h)):
            nd = self.lib.mkd_parser_param_shape(self._h, i, shp)
            out[self.lib.mkd_parser_param_name(self._h, i).decode()] = tuple(int(shp[k]) for k in range(nd))
        return out

    def param_count(self) -> int:
        return int(self.lib.mkd_parser_param_count(self._h))

    def load_weight(self, name: str, t) -> None:
        a = np.ascontiguousarray(t.detach().float().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32))
        shp = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        _lib.check(self.lib.mkd_parser_load_weight(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.ndim, shp), f'mkd_parser_load_weight({name})')
        self.finalized = False

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> 'FaceParser':
        """upstream's names; the training-only heads (conv_out16.*, conv_out32.*) and *.num_batches_tracked are ignored by the library.
        strict: every expected tensor must be there and no other."""
        exp = self.expected_params()
        if strict:
            ignorable = lambda k: k.startswith(('conv_out16.', 'conv_out32.')) or k.endswith('num_batches_tracked')
            missing = [k for k in exp if k not in sd]
            extra = [k for k in sd if k not in exp and not ignorable(k)]
            if missing or extra:
                raise KeyError(f'face parser state dict: missing {missing[:5]}, unexpected {extra[:5]}')
        for k, v in sd.items():
            if k in exp or strict:
                self.load_weight(k, v)
        return self

    def load(self, path: str) -> 'FaceParser':
        """a plain ``torch.load`` state dict (upstream's 79999_iter.pth layout)"""
        sd = torch.load(path, map_location='cpu')
        if isinstance(sd, dict) and 'state_dict' in sd and not any(k.startswith('cp.') for k in sd):
            sd = sd['state_dict']
        return self.load_state_dict(sd)

    def init_random(self, seed: int = 0) -> 'FaceParser':
        """weights for tests and timing runs: He-normal convolutions, BatchNorm statistics near the identity"""
        g = torch.Generator().manual_seed(int(seed))
        for name, shape in self.expected_params().items():
            if name.endswith('running_var'):
                t = 0.5 + torch.rand(shape, generator=g)
            elif name.endswith('running_mean') or name.endswith('.bias'):
                t = 0.4 * torch.rand(shape, generator=g) - 0.2
            elif len(shape) == 1:
                t = 0.8 + 0.4 * torch.rand(shape, generator=g)
            else:
                t = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
            self.load_weight(name, t)
        return self

    def finalize(self) -> 'FaceParser':
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_parser_finalize(self._h), 'mkd_parser_finalize')
        self.finalized = True
        return self

    # ---- inference ----------------------------------------------------------------------------------------
    def _images(self, img01: torch.Tensor) -> torch.Tensor:
        if not isinstance(img01, torch.Tensor) or img01.dim() != 4 or img01.shape[1] != 3:
            raise ValueError(f'images must be [B,3,H,W] in [0, 1], got {tuple(getattr(img01, "shape", ()))}')
        return img01.to(device=self.device, dtype=torch.float32).contiguous()

    def logits(self, img01: torch.Tensor) -> torch.Tensor:
        """[B,3,H,W] in [0,1] -> fp32 logits [B,n_classes,H/8,W/8]"""
        x = self._images(img01)
        B, _, H, W = (int(v) for v in x.shape)
        out = torch.empty((B, self.cfg.n_classes, max(H // 8, 1), max(W // 8, 1)), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_parser_logits(self._h, C.c_void_p(x.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()), C.c_void_p(_stream())),
                       'mkd_parser_logits')
        return out

    def parse(self, img01: torch.Tensor, out_size=None, lut=LUT_SEG, return_logits: bool = False):
        """[B,3,H,W] in [0,1] -> labels uint8 [B,out_h,out_w] (``out_size`` an int or (h, w); default: the images' size), remapped by
        ``lut`` (None: upstream's classes).  return_logits: (labels, logits [B,n_classes,H/8,W/8])."""
        x = self._images(img01)
        B, _, H, W = (int(v) for v in x.shape)
        if out_size is None:
            out_h, out_w = H, W
        elif isinstance(out_size, int):
            out_h = out_w = int(out_size)
        else:
            out_h, out_w = (int(v) for v in out_size)
        labels = torch.empty((B, max(out_h, 0), max(out_w, 0)), device=self.device, dtype=torch.uint8)
        lg = torch.empty((B, self.cfg.n_classes, max(H // 8, 1), max(W // 8, 1)), device=self.device, dtype=torch.float32) if return_logits else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mkd_parser_parse(self._h, C.c_void_p(x.data_ptr()), B, H, W, out_h, out_w, _check_lut(lut, self.cfg.n_classes),
                                                 C.c_void_p(labels.data_ptr()), C.c_void_p(None if lg is None else lg.data_ptr()),
                                                 C.c_void_p(_stream())), 'mkd_parser_parse')
        return (labels, lg) if return_logits else labels

    def find_boxes(self, photos, grow: float = 1.0, parse_size: int = 512, lut=LUT_SEG) -> List[Tuple[int, int, int, int]]:
        return find_boxes(self, photos, grow=grow, parse_size=parse_size, lut=lut)

    def find_faces(self, photos, max_faces: int = 8, min_area: Optional[int] = None, grow: float = 1.0, parse_size: int = 512,
                   lut=LUT_SEG, return_owner: bool = False, oriented: bool = False, min_roll: float = 5.0):
        return find_faces(self, photos, max_faces=max_faces, min_area=min_area, grow=grow, parse_size=parse_size, lut=lut,
                          return_owner=return_owner, oriented=oriented, min_roll=min_roll)

    def flops(self, H: int = 512, W: int = 512) -> float:
        return float(self.lib.mkd_parser_flops(self._h, int(H), int(W)))

    def launches(self) -> int:
        return int(self.lib.mkd_parser_launches(self._h))

    def close(self) -> None:
        if getattr(self, '_h', None):
            self.lib.mkd_parser_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_label_box(labels: torch.Tensor, classes: Sequence[int] = FACE_CLASSES) -> Tuple[int, int, int, int]:
    """(row min, row max, col min, col max), inclusive, of the pixels of one [H,W] device label map whose label is in ``classes``: the
    box mkd_region_mask_from_labels returns (what photo.square_box_from_labels grows); row max < row min when there is none"""
    from . import makeup_score as ms
    _, _, box = ms.region_mask(labels[None], classes, box_classes=classes, margin=0)
    return tuple(int(v) for v in box[0].tolist())


def _squash_parse(parser, chunk, S: int, lut, resize) -> torch.Tensor:
    """whole photos squashed to S x S (``resize``: photo.crop_resize of the whole photo) and parsed -> their label maps [n,S,S]"""
    whole = [(0, 0, int(p.shape[1]), int(p.shape[0])) for p in chunk]
    return parser.parse(resize(chunk, whole, S).img01, out_size=None, lut=lut)


def _scale_box(box, S: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """(row min, row max, col min, col max), inclusive, on the S x S squashed map of an H x W photo -> photo pixels, outwards"""
    r0, r1, c0, c1 = box
    return r0 * H // S, min(H, -(-(r1 + 1) * H // S)) - 1, c0 * W // S, min(W, -(-(c1 + 1) * W // S)) - 1


def find_boxes(parser, photos, grow: float = 1.0, parse_size: int = 512, lut=LUT_SEG, classes: Sequence[int] = FACE_CLASSES,
               resize=None, box_of=None) -> List[Tuple[int, int, int, int]]:
    """Face boxes (x0, y0, side, side) for whole photos (uint8 [H,W,3] device tensors): every photo is squashed to parse_size x
    parse_size (photo.crop_resize of the whole photo), parsed, the bounding box of the face classes (mkd_region_mask_from_labels, as
    in photo.square_box_from_labels) is scaled back to photo pixels (outwards) and grown, squared and clipped by
    photo.grow_square_box -- the box is scaled BEFORE it is grown because the squash changes the aspect ratio.  For localisation
    only: a photo is taken to show ONE face (the box spans every face pixel).  A photo with no face pixel raises ValueError naming
    its index.  This rule is this build's.  ``parser`` is anything with ``parse(img01, out_size=None, lut=...)``; ``resize`` and
    ``box_of`` replace the two device calls (tests of the box arithmetic without a device)."""
    from . import photo
    photos = photo.as_list(photos, 3)
    resize = resize or photo.crop_resize
    box_of = box_of or device_label_box
    S = int(parse_size)
    out = []
    for b0 in range(0, len(photos), MAX_BATCH):
        chunk = photos[b0:b0 + MAX_BATCH]
        labels = _squash_parse(parser, chunk, S, lut, resize)
        for i, (p, l) in enumerate(zip(chunk, labels)):
            H, W = int(p.shape[0]), int(p.shape[1])
            box = box_of(l, classes)
            if box[1] < box[0] or box[3] < box[2]:
                raise ValueError(f'find_boxes: photo {b0 + i} has no pixel of the face classes {tuple(classes)}')
            out.append(photo.grow_square_box(_scale_box(box, S, H, W), H, W, grow))
    return out


def find_faces(parser, photos, max_faces: int = 8, min_area: Optional[int] = None, grow: float = 1.0, parse_size: int = 512, lut=LUT_SEG,
               classes: Sequence[int] = FACE_CLASSES, resize=None, components_of=None, return_owner: bool = False, owner_of=None,
               oriented: bool = False, min_roll: float = 5.0, frames_of=None):
    """EVERY face of whole photos (uint8 [H,W,3] device tensors): one list of boxes (x0, y0, side, side) per photo, largest face first.
    Every photo is squashed to parse_size x parse_size and parsed exactly as find_boxes does; a face is an 8-connected component of the
    face classes with at least ``min_area`` pixels of the squashed map (components.label_components; default (parse_size // 32)^2,
    which drops parser speckle); the ``max_faces`` largest are kept in the table's order (area descending, ties by the smallest
    linear index).  Each component's box is scaled back to photo pixels with find_boxes' expression (outwards, BEFORE it is grown:
    the squash changes the aspect ratio) and grown, squared and clipped by photo.grow_square_box.  A photo without such a component
    gives [] and does not raise.  One device-to-host copy (table and count together) per chunk of MAX_BATCH photos; no component
    data is read back per pixel.  The crop of one face may show part of a neighbouring face: crops are not restricted to their
    component; what keeps one face's PASTE off its neighbour is the owner map.  ``return_owner``: (faces, owner) with owner uint8
    [n_photos, parse_size, parse_size] on the device, the rank of the component nearest to every pixel of the squashed map
    (components.owner_map; components.NO_OWNER in a photo without a face).  The table is then taken with max_out =
    components.MAX_OUT: its first ``max_faces`` rows are the rows of the call above, so the boxes are the same, and EVERY row is a
    seed, so a face beyond ``max_faces`` keeps its pixels.  The metric is the squashed map's: anisotropic in photo pixels.  This rule
    is this build's.  ``resize``, ``components_of`` (the signature of components.label_components) and ``owner_of`` (that of
    components.owner_map) replace the device calls (tests of the box arithmetic without a device).

    ``oriented``: photo.Frame's (cx, cy, side, c, s) instead of boxes; ranks, table order and owner map are unchanged.  Every
    component's roll is measured on the device from the two eye classes (components.face_frames: labels 4 and 5 of ``lut``), which
    needs the component ids, so the table is taken with want_ids.  A face whose measured |roll| is below ``min_roll`` degrees -- also
    one without two eyes or rolled beyond 60 degrees, which measure as 0 -- gets EXACTLY the frame of its box above,
    photo.frame_from_box(photo.grow_square_box(...)): upright faces crop as before.  Any other face gets photo.grow_frame of its row:
    the reference's ratios applied in the face's own frame.  ``frames_of`` (the signature of components.face_frames) replaces the
    device call.  Still one device-to-host copy per chunk: the frames travel with the table."""
    from . import components, photo
    K = int(max_faces)
    if K != max_faces or not 1 <= K <= components.MAX_OUT:
        raise ValueError(f'max_faces must be an integer 1..{components.MAX_OUT}, got {max_faces!r}')
    photos = photo.as_list(photos, 3)
    resize = resize or photo.crop_resize
    components_of = components_of or components.label_components
    S = int(parse_size)
    area = (S // 32) ** 2 if min_area is None else int(min_area)
    if area < 1:
        raise ValueError(f'min_area must be >= 1, got {min_area!r} (parse_size {parse_size})')
    if return_owner:
        owner_of = owner_of or components.owner_map
    if oriented:
        frames_of = frames_of or components.face_frames
        if not float(min_roll) >= 0.0:
            raise ValueError(f'min_roll must be >= 0 degrees, got {min_roll!r}')
    out: List[List[Tuple[int, int, int, int]]] = []
    owners = []
    for b0 in range(0, len(photos), MAX_BATCH):
        chunk = photos[b0:b0 + MAX_BATCH]
        labels = _squash_parse(parser, chunk, S, lut, resize)
        if return_owner:
            table, count, ids = components_of(labels, classes, min_area=area, max_out=components.MAX_OUT, want_ids=True)
            owners.append(torch.as_tensor(owner_of(ids, table)))
        elif oriented:
            table, count, ids = components_of(labels, classes, min_area=area, max_out=K, want_ids=True)
        else:
            table, count = components_of(labels, classes, min_area=area, max_out=K)[:2]
        table, count = torch.as_tensor(table), torch.as_tensor(count)
        parts = [table.reshape(len(chunk), -1), count.reshape(len(chunk), 1).to(table.dtype)]
        rows = int(table.shape[1])
        if oriented:
            fr = torch.as_tensor(frames_of(labels, ids, table, [(int(p.shape[0]), int(p.shape[1])) for p in chunk]))
            parts = [t.to(torch.int64) for t in parts] + [fr.reshape(len(chunk), -1).to(torch.int64)]
        both = torch.cat(parts, 1).cpu().tolist()
        for p, row in zip(chunk, both):
            H, W = int(p.shape[0]), int(p.shape[1])
            faces = []
            for k in range(min(int(row[6 * rows]), K)):
                box = photo.grow_square_box(_scale_box(row[6 * k + 2:6 * k + 6], S, H, W), H, W, grow)
                if oriented:
                    frow = row[6 * rows + 1 + 8 * k:6 * rows + 9 + 8 * k]
                    rolled = abs(photo.frame_roll(frow)) >= float(min_roll) and (frow[2], frow[3]) != (components.FRAME_UNIT, 0)
                    faces.append(photo.grow_frame(frow, S, H, W, grow) if rolled else photo.frame_from_box(box))
                else:
                    faces.append(box)
            out.append(faces)
    if return_owner:
        return out, (torch.cat(owners) if owners else torch.empty((0, S, S), dtype=torch.uint8))
    return out
