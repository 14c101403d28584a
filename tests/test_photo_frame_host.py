"""CPU: the restatement of the tilted-face calls (tests/photo_frame_ref.py) against the rules the repository already has (Pillow's
bytes, the axis-aligned paste, a rotated photo), its properties, photo.grow_frame and face_parser.find_faces(oriented=True) with
their device calls stubbed, the library's argument checks (they run before anything is enqueued, so they need no device),
photo.read_boxes_multi's six-field lines and the flags of runs/test.py."""
import ctypes as C
import importlib.util
import math
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import components_ref as cr
import photo_frame_ref as fr
import photo_ref as pr
from makeupdiffuse_amd import components
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import photo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'photo_resize.npz'))
PHOTOS = [GOLDEN[f'photo{i}'] for i in range(4)]          # 150 x 203, 97 x 64, 64 x 64, 40 x 200


def box_frame(box):
    x0, y0, bw, bh = box
    return (x0 + bw / 2.0, y0 + bh / 2.0, float(bw), 1.0, 0.0)


# ---- the restatement against the existing rules ---------------------------------------------------------------------------------------
# integer square boxes strictly inside their photo, far enough for the filter's support (max(scale, 1) pixels beyond the box) to stay
# inside too: enlarging, scale 1, reducing by non-integers.  Where the support leaves the photo the two rules differ BY DESIGN: Pillow
# drops the taps outside and renormalises, the frame crop replicates the edge (a rotated square has no other choice); that rule has
# its own test below
CROP_CASES = [(0, (20, 10, 100, 100), 37), (0, (50, 40, 16, 16), 16), (0, (10, 10, 120, 120), 16), (1, (5, 20, 50, 50), 64), (1, (2, 2, 60, 60), 37),
              (2, (10, 12, 37, 37), 37), (2, (8, 8, 48, 48), 8), (3, (80, 3, 34, 34), 16)]


@pytest.mark.parametrize('k', range(len(CROP_CASES)))
def test_upright_crop_is_pillows_within_one(k):
    """Pillow rounds its horizontal pass to uint8 (at most 0.5 off) and filters that vertically with weights that sum to one, so its
    value before the last rounding is within 0.5 (+ 2^-22 fixed-point coefficient error times 255 per tap, far below the rest) of the
    exact separable filter, which is the frame's filter at roll 0; two roundings of values at most 0.5 apart differ by at most 1."""
    i, box, S = CROP_CASES[k]
    want = pr.crop_resize_u8(PHOTOS[i], box, S)
    H, W = PHOTOS[i].shape[:2]
    reach = max(box[2] / S, 1.0)
    assert box[0] >= reach and box[1] >= reach and box[0] + box[2] + reach <= W and box[1] + box[3] + reach <= H
    got, _, _ = fr.crop_frame(PHOTOS[i], box_frame(box), S)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert (got != want).mean() < 0.5


@pytest.mark.parametrize('angle', [0.0, 33.0])
def test_crop_replicates_the_photos_edges(angle):
    """a square that sticks out of the photo reads what an edge-padded photo holds there: the same taps in the same order, so equal"""
    ph, pad = PHOTOS[2], 40
    big = np.pad(ph, ((pad, pad), (pad, pad), (0, 0)), mode='edge')
    got, _, _ = fr.crop_frame(ph, fr.frame(6, 60, 44, angle), 16)
    want, _, _ = fr.crop_frame(big, fr.frame(6 + pad, 60 + pad, 44, angle), 16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('rho', [0, 3, 8])
def test_upright_paste_is_the_axis_aligned_paste_within_one(rho):
    ph, box, S = PHOTOS[0], (30, 20, 90, 90), 16
    g = np.random.default_rng(41 + rho)
    s01 = g.random((3, S, S)).astype(np.float32)
    t = g.uniform(-1.5, 1.5, s01.shape).astype(np.float32)
    want = pr.paste(ph, box, t, s01, rho)
    got, _, inside = fr.paste_frame(ph, box_frame(box), t, s01, rho)
    x0, y0, bw, bh = box
    assert inside.sum() == bw * bh and inside[y0:y0 + bh, x0:x0 + bw].all()
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1 and not np.array_equal(got, ph)


@pytest.mark.parametrize('i,cx,cy,side,S', [(0, 100.0, 70.0, 80.0, 37), (1, 30.5, 50.25, 40.0, 16), (3, 150.0, 20.0, 36.0, 16)])
def test_quarter_turn_crop_is_the_upright_crop_of_the_rotated_photo(i, cx, cy, side, S):
    """e_u = (0, 1): out[i][j] samples the photo at (cx - v_i, cy + u_j).  np.rot90(photo) [r][c] = photo[c][W - 1 - r], so a point
    (x', y') of the rotated photo is the point (W - y', x') of the photo: the same samples, summed in another order."""
    ph = PHOTOS[i]
    W = ph.shape[1]
    got, _, _ = fr.crop_frame(ph, (cx, cy, side, 0.0, 1.0), S)
    want, _, _ = fr.crop_frame(np.ascontiguousarray(np.rot90(ph)), (cy, W - cx, side, 1.0, 0.0), S)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    assert not np.array_equal(got, fr.crop_frame(ph, (cx, cy, side, 1.0, 0.0), S)[0])


def test_crop_labels_are_sampled_not_interpolated():
    ph = PHOTOS[2]
    lab = (np.arange(64)[:, None] // 8 * 8 + np.arange(64)[None, :] // 8).astype(np.uint8)
    _, _, got = fr.crop_frame(ph, fr.frame(30, 33, 50, 17.0), 16, lab)
    assert got.shape == (16, 16) and set(np.unique(got)) <= set(np.unique(lab))


# ---- properties of the paste ----------------------------------------------------------------------------------------------------------
FRAMES = [fr.frame(60, 40, 50, 17.0), fr.frame(5, 3, 40, -30.0), fr.frame(64, 97, 30, 45.0), fr.frame(-8.0, 50, 24, 90.0), fr.frame(32.5, 48.25, 61.3, 0.0)]


@pytest.fixture(scope='module')
def paste_inputs():
    g = np.random.default_rng(977)
    s01 = g.random((3, 16, 16)).astype(np.float32)
    return s01, g.uniform(-2.0, 2.0, s01.shape).astype(np.float32)


@pytest.mark.parametrize('k', range(len(FRAMES)))
def test_paste_properties(paste_inputs, k):
    s01, t = paste_inputs
    ph = PHOTOS[1]
    H, W = ph.shape[:2]
    f = FRAMES[k]
    same, _, _ = fr.paste_frame(ph, f, (2.0 * s01 - 1.0).astype(np.float32), s01, 3)
    assert np.array_equal(same, ph)                                              # t = 2 s01 - 1: no difference to paste
    got, _, inside = fr.paste_frame(ph, f, t, s01, 3)
    assert np.array_equal(inside, fr.inside_mask(H, W, f)) and 0 < inside.sum() < H * W
    assert np.array_equal(got[~inside], ph[~inside]) and (got[inside] != ph[inside]).mean() > 0.3
    ones, _, _ = fr.paste_frame(ph, f, t, s01, 3, np.ones((7, 5), np.float32))
    assert np.array_equal(ones, got)                                             # a * 1 is a
    zeros, _, _ = fr.paste_frame(ph, f, t, s01, 3, np.zeros((5, 9), np.float32))
    assert np.array_equal(zeros, ph)
    w = np.zeros((H, W), np.float32)
    w[:, W // 2:] = 1.0                                                          # at the photo's own resolution: a 0 / 1 plane
    part, _, _ = fr.paste_frame(ph, f, t, s01, 3, w)
    assert np.array_equal(part[:, :W // 2], ph[:, :W // 2]) and np.array_equal(part[:, W // 2:], got[:, W // 2:])


# ---- grow_frame and find_faces(oriented=True) ---------------------------------------------------------------------------------------
Cropped = namedtuple('Cropped', 'img01 labels u8')


class StubParser:
    def __init__(self, maps):
        self.maps = maps

    def parse(self, img01, out_size=None, lut=None):
        return self.maps[:img01.shape[0]]


def stub_resize(photos, boxes, size):
    return Cropped(torch.zeros(len(photos), 3, size, size), None, None)


def host_components(labels, classes, min_area=1, max_out=16, want_ids=False):
    t, c, ids = cr.label_components(labels.numpy(), classes, min_area, max_out)
    return torch.from_numpy(t), torch.from_numpy(c), torch.from_numpy(ids) if want_ids else None


def host_frames(seen=None):
    def frames_of(labels, ids, table, photo_hw, classes_a=(4,), classes_b=(5,), min_eye_area=None):
        out = fr.face_frames(labels.numpy(), ids.numpy(), table.numpy(), photo_hw, classes_a, classes_b, min_eye_area)
        if seen is not None:
            seen.append(out)
        return torch.from_numpy(out)
    return frames_of


def host_owner(ids, table):
    return torch.zeros(ids.shape, dtype=torch.uint8)


def photo_roll(roll_deg, H, W):
    """a roll on the square squashed map, seen in the H x W photo"""
    return math.degrees(math.atan2(math.sin(math.radians(roll_deg)) * H, math.cos(math.radians(roll_deg)) * W))


def test_two_rolled_faces_come_back_with_their_roll():
    S = 64
    maps = torch.from_numpy(np.stack([fr.two_faces(S), fr.two_faces(S)]))
    photos = [torch.zeros(640, 640, 3, dtype=torch.uint8), torch.zeros(480, 800, 3, dtype=torch.uint8)]
    seen = []
    got = fp.find_faces(StubParser(maps), photos, parse_size=S, resize=stub_resize, components_of=host_components, frames_of=host_frames(seen),
                        oriented=True)
    boxes = fp.find_faces(StubParser(maps), photos, parse_size=S, resize=stub_resize, components_of=host_components)
    assert len(seen) == 1 and seen[0].shape == (2, 8, 8)                        # one call per chunk, the table's rows
    for p, faces, bx in zip(photos, got, boxes):
        H, W = int(p.shape[0]), int(p.shape[1])
        assert len(faces) == 2 and len(bx) == 2                                  # ranks and order are those of the boxes
        for f, (x, y, want) in zip(faces, fr.TWO_FACES):
            assert isinstance(f, photo.Frame) and abs(f.c * f.c + f.s * f.s - 1.0) < 1e-12
            assert abs(math.degrees(math.atan2(f.s, f.c)) - photo_roll(want, H, W)) <= 2.0
            assert 0 < f.side <= min(H, W)
            # the face's centre lies well inside the frame, above its middle (the crop leaves more room above a face than below)
            rx, ry = x * W / S - f.cx, y * H / S - f.cy
            u, v = f.c * rx + f.s * ry, -f.s * rx + f.c * ry
            assert abs(u) < f.side / 8 and 0 < v < f.side / 4
    # rows beyond the faces are fill rows
    assert (seen[0][:, 2:, :4] == np.array([0, 0, fr.UNIT, 0])).all() and (seen[0][:, 2:, 4] == fr.INT64_MAX).all()
    # with the owner map the table has MAX_OUT rows: the same frames
    both, owner = fp.find_faces(StubParser(maps), photos, parse_size=S, resize=stub_resize, components_of=host_components,
                                frames_of=host_frames(), oriented=True, return_owner=True, owner_of=host_owner)
    assert both == got and tuple(owner.shape) == (2, S, S)


def test_grow_frame_holds_the_whole_face_and_applies_the_ratios_in_the_faces_frame():
    S, H, W = 64, 512, 512
    lab = np.zeros((S, S), np.uint8)
    fr.draw_face(lab, 32, 32, 10, 14, 30.0)
    t, _, ids = cr.label_components(lab[None], fp.FACE_CLASSES, 1, 1)
    row = fr.face_frames(lab[None], ids, t, [(H, W)])[0, 0]
    assert abs(photo.frame_roll(row) - 30.0) <= 2.0
    f0 = photo.grow_frame(row, S, H, W, grow=0.0)
    k = H / S
    # without growing: the rolled ellipse's own extents, 2 * 10 and 2 * 14 squashed pixels, the longer one as the side (within a pixel
    # of the squashed map, the centres' extent being widened by half a pixel's footprint per side)
    assert abs(f0.side - 28 * k) <= 1.5 * k and abs(f0.cx - 32 * k) <= k and abs(f0.cy - 32 * k) <= k
    f1 = photo.grow_frame(row, S, H, W, grow=1.0)
    assert abs(f1.side - 28 * k * (1 + 0.8 / 0.85)) <= 3 * k
    # the centre moves UP IN THE FACE'S FRAME by (0.6 - 0.2) / 0.85 / 2 of the height: along -e_v = (s, -c)
    shift = (photo.UP_RATIO - photo.DOWN_RATIO) / 2 * (f0.side)
    assert abs((f1.cx - f0.cx) - shift * f1.s) <= k and abs((f1.cy - f0.cy) + shift * f1.c) <= k
    assert photo.grow_frame(row, S, 64, 64, grow=4.0).side == 64.0           # limited to the photo's shorter side
    for bad in (list(row[:7]), [0, 0, fr.UNIT, 0, fr.INT64_MAX, fr.INT64_MIN, fr.INT64_MAX, fr.INT64_MIN]):
        with pytest.raises(ValueError):
            photo.grow_frame(bad, S, H, W)


def test_upright_one_eyed_and_overrolled_faces_keep_their_boxes_bit_for_bit():
    S = 64
    one_eye, slight, over = np.zeros((S, S), np.uint8), np.zeros((S, S), np.uint8), np.zeros((S, S), np.uint8)
    fr.draw_face(one_eye, 30, 30, 12, 16, 25.0, eyes=(True, False))
    fr.draw_face(slight, 34, 30, 12, 16, 3.0)
    fr.draw_face(over, 32, 32, 12, 16, 75.0)
    maps = torch.from_numpy(np.stack([one_eye, slight, over]))
    photos = [torch.zeros(300, 200, 3, dtype=torch.uint8), torch.zeros(512, 512, 3, dtype=torch.uint8), torch.zeros(256, 256, 3, dtype=torch.uint8)]
    seen = []
    got = fp.find_faces(StubParser(maps), photos, parse_size=S, resize=stub_resize, components_of=host_components, frames_of=host_frames(seen),
                        oriented=True, min_roll=5.0)
    boxes = fp.find_faces(StubParser(maps), photos, parse_size=S, resize=stub_resize, components_of=host_components)
    rows = seen[0][:, 0]
    assert rows[0][1] == 0 and tuple(rows[0][2:4]) == (fr.UNIT, 0)              # the missing eye: no direction
    assert 0 < abs(photo.frame_roll(rows[1])) < 5.0                             # measured, but below min_roll
    assert tuple(rows[2][2:4]) == (fr.UNIT, 0) and rows[2][0] > 0 and rows[2][1] > 0          # 75 degrees: taken as a parser error
    for faces, bx in zip(got, boxes):
        assert faces == [photo.frame_from_box(bx[0])] and photo.box_from_frame(faces[0]) == bx[0]
        assert faces[0].s == 0.0 and faces[0].c == 1.0
    # min_roll 0 lets the slight roll through
    loose = fp.find_faces(StubParser(maps), photos, parse_size=S, resize=stub_resize, components_of=host_components, frames_of=host_frames(),
                          oriented=True, min_roll=0.0)
    assert loose[1][0].s != 0.0 and loose[0] == got[0] and loose[2] == got[2]
    with pytest.raises(ValueError, match='min_roll'):
        fp.find_faces(StubParser(maps), photos, parse_size=S, resize=stub_resize, components_of=host_components, frames_of=host_frames(),
                      oriented=True, min_roll=-1.0)


def test_eyes_below_min_eye_area_give_no_direction():
    S = 64
    lab = np.zeros((S, S), np.uint8)
    fr.draw_face(lab, 32, 32, 12, 16, 25.0)
    t, _, ids = cr.label_components(lab[None], fp.FACE_CLASSES, 1, 2)
    n = int(min((lab == 4).sum(), (lab == 5).sum()))
    assert tuple(fr.face_frames(lab[None], ids, t, [(64, 64)], min_eye_area=n)[0, 0, 2:4]) != (fr.UNIT, 0)
    assert tuple(fr.face_frames(lab[None], ids, t, [(64, 64)], min_eye_area=n + 1)[0, 0, 2:4]) == (fr.UNIT, 0)


def test_frame_from_box_and_back():
    f = photo.frame_from_box((10, 20, 30, 30))
    assert f == photo.Frame(25.0, 35.0, 30.0, 1.0, 0.0) and photo.box_from_frame(f) == (10, 20, 30, 30)
    assert photo.frame_from_box((10, 20, 30, 30), 90.0)[3:] == (0.0, 1.0) and photo.frame_from_box((10, 20, 30, 30), -90.0)[3:] == (0.0, -1.0)
    assert photo.frame_from_box((10, 20, 30, 30), 180.0)[3:] == (-1.0, 0.0)
    g = photo.frame_from_box((10, 20, 31, 31), 30.0)
    assert g[:3] == (25.5, 35.5, 31.0) and abs(g.c - math.cos(math.pi / 6)) < 1e-15 and abs(g.s - 0.5) < 1e-15
    assert photo.box_from_frame(g) is None and photo.box_from_frame(photo.Frame(25.25, 35.0, 30.0, 1.0, 0.0)) is None
    assert photo.box_from_frame(photo.frame_from_box((10, 20, 31, 31))) == (10, 20, 31, 31)
    for box, angle in (((0, 0, 30, 20), 10.0), ((0, 0, 30, 20), 0.0), ((0, 0, 0, 0), 0.0), ((0, 0, 8, 8), math.inf), ((0, 0, 8), 0.0)):
        with pytest.raises(ValueError):
            photo.frame_from_box(box, angle)
    bi, boxes, fi, frames = photo.split_regions([(1, 2, 3, 4), g, f])
    assert (bi, boxes, fi, frames) == ([0, 2], [(1, 2, 3, 4), (10, 20, 30, 30)], [1], [g])


def test_check_frame_limits():
    ok = photo.check_frame((50.0, 40.0, 30.0, 0.6, 0.8), 100, 120, 16)
    assert ok == photo.Frame(50.0, 40.0, 30.0, 0.6, 0.8)
    for bad in ((50, 40, 0.0, 1, 0), (50, 40, 16 * 32 + 1, 1, 0), (50, 40, 30, 1, 0.001), (50, 40, math.nan, 1, 0), (-31, 40, 30, 1, 0),
                (50, 131, 30, 1, 0), (151, 40, 30, 1, 0), (50, 40, 30, 1)):
        with pytest.raises(ValueError):
            photo.check_frame(bad, 100, 120, 16)


# ---- the library's argument checks: before anything is enqueued, so without a device ------------------------------------------------
FAKE = 0x10000          # a non-null pointer that is never followed: every call below is refused on the host


def frame_desc(**kw):
    d = (mlib.PhotoFrameDescC * 1)()
    v = dict(pixels=FAKE, pitch_bytes=300, H=80, W=100, cx=50.0, cy=40.0, side=30.0, c=1.0, s=0.0, labels=None)
    v.update(kw)
    for k, x in v.items():
        setattr(d[0], k, x)
    return d


BAD_DESCS = [dict(pixels=None), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(pitch_bytes=299), dict(cx=math.nan), dict(cy=math.inf),
             dict(side=math.nan), dict(c=math.nan, s=0.0), dict(c=1.0, s=-math.inf), dict(side=0.0), dict(side=-1.0), dict(side=32 * 16 + 0.5),
             dict(c=1.0, s=1e-4), dict(c=0.7, s=0.7), dict(cx=-30.5), dict(cx=130.5), dict(cy=-30.5), dict(cy=110.5)]


def test_crop_and_paste_frame_refuse_bad_arguments():
    lib = mlib.load()
    P = C.c_void_p
    S = 16
    crop = lambda d, n=1, S=S, img=FAKE, u8=None, lab=None: lib.mkd_crop_frame(d, n, S, P(img), P(u8), P(lab), None)
    paste = lambda d, n=1, S=S, t=FAKE, s=FAKE, rho=3, w=None, wh=0, ww=0: lib.mkd_paste_frame(d, n, S, P(t), P(s), rho, P(w), wh, ww, None)
    for bad in BAD_DESCS:
        assert crop(frame_desc(**bad)) == -1 and lib.mkd_last_error(), bad
        assert paste(frame_desc(**bad)) == -1 and lib.mkd_last_error(), bad
    good = frame_desc()
    for kw in (dict(n=0), dict(n=17), dict(S=7), dict(S=1025), dict(img=None, u8=None), dict(lab=FAKE)):          # labels_out without a label map
        assert crop(good, **kw) == -1 and lib.mkd_last_error(), kw
    assert lib.mkd_crop_frame(None, 1, S, P(FAKE), None, None, None) == -1
    for kw in (dict(n=0), dict(n=17), dict(S=7), dict(S=1025), dict(t=None), dict(s=None), dict(rho=-1), dict(rho=65), dict(w=FAKE, wh=0, ww=8),
               dict(w=FAKE, wh=8, ww=0), dict(w=FAKE, wh=2049, ww=8), dict(w=FAKE, wh=8, ww=2049)):
        assert paste(good, **kw) == -1 and lib.mkd_last_error(), kw
    assert lib.mkd_paste_frame(None, 1, S, P(FAKE), P(FAKE), 3, None, 0, 0, None) == -1
    # the limits themselves pass the descriptor check: the next check refuses (a message of its own)
    for edge in (dict(side=32.0 * S), dict(cx=-30.0), dict(cy=110.0), dict(c=0.6, s=0.8)):
        assert crop(frame_desc(**edge), img=None) == -1 and b'both null' in lib.mkd_last_error(), edge


def test_face_frames_refuses_bad_arguments():
    lib = mlib.load()
    P = C.c_void_p
    assert lib.mkd_face_frames_scratch_bytes(16, 64) == 16 * 64 * 48 and lib.mkd_face_frames_scratch_bytes(1, 1) == 256
    for b, k in ((0, 4), (17, 4), (2, 0), (2, 65)):
        assert lib.mkd_face_frames_scratch_bytes(b, k) == 0
    hw = (C.c_int32 * 4)(480, 640, 100, 100)
    good = dict(labels=FAKE, ids=FAKE, table=FAKE, batch=2, S=64, max_out=4, hw=hw, area=1, frames=FAKE, scratch=0x10000)
    call = lambda a: lib.mkd_face_frames(P(a['labels']), P(a['ids']), P(a['table']), a['batch'], a['S'], a['max_out'], a['hw'], C.c_uint64(1 << 4),
                                         C.c_uint64(1 << 5), a['area'], P(a['frames']), P(a['scratch']), None)
    for bad in (dict(batch=0), dict(batch=17), dict(S=0), dict(S=4097), dict(max_out=0), dict(max_out=65), dict(area=0), dict(labels=None),
                dict(ids=None), dict(table=None), dict(hw=None), dict(frames=None), dict(scratch=None), dict(scratch=0x10010),
                dict(hw=(C.c_int32 * 4)(0, 640, 100, 100)), dict(hw=(C.c_int32 * 4)(480, 640, 100, 16385)), dict(hw=(C.c_int32 * 4)(480, 640, 16385, 1))):
        assert call(dict(good, **bad)) == -1 and lib.mkd_last_error(), bad
    assert lib.mkd_abi_version() == 1


def test_python_side_checks_need_no_device():
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    ids = torch.zeros(2, 8, 8, dtype=torch.int32)
    table = torch.zeros(2, 4, 6, dtype=torch.int32)
    with pytest.raises(mlib.MkdError, match='HIP device'):
        components.face_frames(lab, ids, table, [(8, 8), (8, 8)])
    for bad in (dict(labels=lab.int()), dict(labels=lab[:, :, :4]), dict(ids=ids.long()), dict(ids=ids[:1]), dict(table=table[:, :, :5]),
                dict(table=torch.zeros(2, 65, 6, dtype=torch.int32))):
        a = dict(labels=lab, ids=ids, table=table)
        a.update(bad)
        with pytest.raises(ValueError):
            components.face_frames(a['labels'], a['ids'], a['table'], [(8, 8), (8, 8)])
    p = torch.zeros(20, 30, 3, dtype=torch.uint8)
    with pytest.raises(mlib.MkdError, match='HIP device'):
        photo.crop_frames([p], [(15.0, 10.0, 8.0, 1.0, 0.0)], 8)
    with pytest.raises(mlib.MkdError, match='HIP device'):
        photo.paste_frames([p], [(15.0, 10.0, 8.0, 1.0, 0.0)], torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


# ---- boxes files and runs/test.py ---------------------------------------------------------------------------------------------------
def test_read_boxes_multi_takes_an_angle_as_sixth_field(tmp_path):
    f = tmp_path / 'boxes.txt'
    f.write_text('# group\na.png 1 2 30 30 12.5\na.png 40 2 20 20\nb.png 0 0 8 8 -90\n')
    got = photo.read_boxes_multi(str(f))
    assert got == {'a.png': [(1, 2, 30, 30, 12.5), (40, 2, 20, 20)], 'b.png': [(0, 0, 8, 8, -90.0)]}
    assert photo.read_boxes(str(f))['a.png'] == (1, 2, 30, 30, 12.5)
    for line in ('a.png 1 2 30 30 x', 'a.png 1 2 30 30 nan', 'a.png 1 2 30 30 1 2', 'a.png 1 2 30'):
        f.write_text(line + '\n')
        with pytest.raises(ValueError):
            photo.read_boxes_multi(str(f))


def test_runs_test_align_flags(monkeypatch, tmp_path):
    spec = importlib.util.spec_from_file_location('runs_test_cli_align', os.path.join(ROOT, 'runs', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.build_parser().parse_args([])
    assert args.align_faces is False and args.min_roll == 5.0
    args = mod.build_parser().parse_args(['--photos', '--max-faces', '3', '--align-faces', '--min-roll', '2.5'])
    assert args.align_faces is True and args.min_roll == 2.5

    def refused(*argv):
        monkeypatch.setattr(sys, 'argv', ['test.py', *argv])
        with pytest.raises(SystemExit) as e:
            mod.main()
        return str(e.value)

    root = str(tmp_path)
    assert '--align-faces only applies with --photos --max-faces' in refused('--align-faces')
    assert '--align-faces only applies with --photos --max-faces' in refused('--align-faces', '--photos', '--data-root', root, '--face-parser', 'random')
    assert '--min-roll only applies with --align-faces' in refused('--min-roll', '3')
    assert '--min-roll only applies with --align-faces' in refused('--min-roll', '3', '--photos', '--data-root', root, '--max-faces', '2',
                                                                   '--face-parser', 'random')
    assert '--min-roll must be >= 0' in refused('--align-faces', '--min-roll', '-1', '--photos', '--data-root', root, '--max-faces', '2',
                                                '--face-parser', 'random')


# ---- the device cases hold no rint tie: tests/test_gpu_photo_frame.py may then ask for EQUAL bytes ---------------------------------------
FRAME_RUNS = [(4, None), (1, None), (4, 20)]          # (max_out, min_eye_area) of the mkd_face_frames cases


def test_device_cases_are_clear_of_rint_ties():
    """A byte of the device can differ from the restatement's only where a value before rint lies at k + 0.5 and a last-bit difference
    (there is none by construction, but a division or a square root could have one) tips it.  No such value comes nearer than 1e-9
    in any crop or paste case, and no direction nearer than 1e-6 in any mkd_face_frames case."""
    ph = fr.case_photos()
    crop = min(fr.tie_margin(fr.crop_frame(ph[p], f, S)[1]) for S in fr.CASE_SIZES for p, f in fr.case_frames(S) + fr.extra_frames(S))
    assert crop > 1e-9, crop
    paste = 1.0
    for S, rho, wt in fr.PASTE_CASES:
        t, s01 = fr.case_samples(S)
        w = fr.case_weights(wt)
        for k, (p, f) in enumerate(fr.case_frames(S)):
            _, o, inside = fr.paste_frame(ph[p], f, t[k], s01[k], rho, None if w is None else w[k])
            assert inside.any()
            paste = min(paste, fr.tie_margin(o[inside]))
    assert paste > 1e-9, paste
    for S in (16, 64):
        lab, hw = fr.frames_maps(S)
        for max_out, area in FRAME_RUNS:
            t, _, ids = cr.label_components(lab, fp.FACE_CLASSES, 1, max_out)
            rows, exact = fr.face_frames(lab, ids, t, hw, min_eye_area=area, want_exact=True)
            e = exact[~np.isnan(exact)]
            assert e.size == 0 or np.abs((e - np.floor(e)) - 0.5).min() > 1e-6
            if S == 64 and area is None and max_out == 4:
                assert (rows[[0, 3, 4], :2, 3] != 0).all() and (rows[2, 0, :2] == 0).all() and rows[1, 0, 4] == fr.INT64_MAX
                assert tuple(rows[0, 0, 2:4]) != tuple(rows[3, 0, 2:4])         # the non-square photo turns the same map's direction
            if S == 64 and area == 20:
                assert rows[0, 0, 3] != 0 and tuple(rows[0, 1, 2:4]) == (fr.UNIT, 0) and rows[0, 1, 0] == 19
