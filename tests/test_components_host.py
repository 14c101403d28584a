"""CPU: the restatement of mkd_label_components (tests/components_ref.py) against scipy.ndimage, the box arithmetic of
face_parser.find_faces with its two device calls stubbed, the library's argument checks (they run before anything is enqueued, so
they need no device), transfer_photos(max_faces=...)'s own checks and photo.read_boxes_multi."""
import ctypes as C
import importlib.util
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import components_ref as cr
from makeupdiffuse_amd import components
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import photo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the restatement against scipy ------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 9), (8, 1), (2, 2), (3, 5), (7, 7), (16, 16), (31, 33), (32, 32), (33, 31), (40, 64), (64, 40), (50, 50), (65, 65), (97, 131),
         (96, 17), (17, 96), (5, 131), (97, 4), (80, 80)]


@pytest.mark.parametrize('k', range(20))
def test_restatement_agrees_with_scipy(k):
    ndi = pytest.importorskip('scipy.ndimage')
    H, W = SIZES[k]
    density = 0.2 + 0.5 * k / 19
    mask = np.random.default_rng(100 + k).random((H, W)) < density
    if k == 0:
        mask[:] = True
    ids, comps = cr.components_of_mask(mask)
    lab, n = ndi.label(mask, structure=np.ones((3, 3)))
    assert n == len(comps)
    assert np.array_equal(ids >= 0, mask)
    if n == 0:
        return
    lin = np.arange(H * W).reshape(H, W)
    low = np.asarray(ndi.minimum(lin, lab, np.arange(1, n + 1))).astype(np.int64).reshape(-1)          # scipy label -> its smallest linear index
    assert np.array_equal(np.where(lab > 0, low[np.maximum(lab, 1) - 1], -1), ids)                       # the same partition, the same ids
    order = np.argsort(low)
    assert np.array_equal(comps[:, 0], low[order])
    area = np.asarray(ndi.sum(mask, lab, np.arange(1, n + 1))).astype(np.int64).reshape(-1)
    assert np.array_equal(comps[:, 1], area[order])
    boxes = ndi.find_objects(lab)
    want = np.array([[boxes[j][0].start, boxes[j][0].stop - 1, boxes[j][1].start, boxes[j][1].stop - 1] for j in order], np.int64).reshape(n, 4)
    assert np.array_equal(comps[:, 2:], want)


def test_restatement_table_order_fill_rows_and_classes():
    lab = np.zeros((12, 20), np.uint8)
    lab[0:2, 0:2] = 1          # area 4, id 0
    lab[5:7, 5:7] = 9          # area 4, id 105
    lab[9:12, 10:16] = 1       # area 18
    lab[0, 19] = 64            # never in
    lab[3, 19] = 5             # not in the class set
    table, count, ids = cr.label_components(lab, (1, 9, 63), min_area=1, max_out=5)
    assert count.tolist() == [3]
    assert table[0].tolist() == [[190, 18, 9, 11, 10, 15], [0, 4, 0, 1, 0, 1], [105, 4, 5, 6, 5, 6], list(cr.FILL_ROW), list(cr.FILL_ROW)]
    assert ids[0, 0, 19] == -1 and ids[0, 3, 19] == -1 and ids[0, 6, 6] == 105
    table, count, _ = cr.label_components(lab, (1, 9), min_area=5, max_out=1)
    assert count.tolist() == [1] and table[0].tolist() == [[190, 18, 9, 11, 10, 15]]
    table, count, _ = cr.label_components(lab, (1, 9), min_area=1, max_out=2)          # count is not capped, the table is cut
    assert count.tolist() == [3] and table[0, :, 0].tolist() == [190, 0]
    assert tuple(cr.FILL_ROW) == tuple(components.FILL_ROW)


# ---- find_faces: the box arithmetic, both device calls stubbed ----------------------------------------------------------------------
Cropped = namedtuple('Cropped', 'img01 labels u8')


class StubParser:
    def __init__(self, maps):
        self.maps, self.calls = maps, []

    def parse(self, img01, out_size=None, lut=None):
        self.calls.append((tuple(img01.shape), out_size, tuple(lut)))
        return self.maps[:img01.shape[0]]


def stub_resize(photos, boxes, size):
    return Cropped(torch.zeros(len(photos), 3, size, size), None, None)


def host_components(seen=None):
    def components_of(labels, classes, min_area=1, max_out=16, want_ids=False):
        if seen is not None:
            seen.append((tuple(labels.shape), tuple(classes), min_area, max_out))
        t, c, _ = cr.label_components(labels.numpy(), classes, min_area, max_out)
        return torch.from_numpy(t), torch.from_numpy(c), None
    return components_of


def host_box(labels, classes):
    m = np.isin(labels.numpy(), list(classes))
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    return (int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])) if len(rows) else (2 ** 31 - 1, -1, 2 ** 31 - 1, -1)


def scaled(box, H, W, S):
    """find_boxes' expression: parse pixels -> photo pixels, outwards"""
    r0, r1, c0, c1 = box
    return (r0 * H // S, min(H, -(-(r1 + 1) * H // S)) - 1, c0 * W // S, min(W, -(-(c1 + 1) * W // S)) - 1)


def test_find_faces_boxes_order_cap_and_empty_photo():
    S = 64
    maps = torch.zeros(3, S, S, dtype=torch.uint8)
    blobs = [(30, 49, 5, 20), (2, 9, 40, 47), (52, 60, 50, 61), (20, 21, 60, 61)]          # areas 320, 64, 108, 4 (rows, cols inclusive)
    for r0, r1, c0, c1 in blobs:
        maps[0, r0:r1 + 1, c0:c1 + 1] = 1
    maps[0, 12:14, 12:14] = 8                                                            # ears: not a face class
    maps[2, 10:30, 10:30] = 7
    photos = [torch.zeros(300, 200, 3, dtype=torch.uint8), torch.zeros(90, 120, 3, dtype=torch.uint8), torch.zeros(64, 64, 3, dtype=torch.uint8)]
    seen, parser = [], StubParser(maps)
    got = fp.find_faces(parser, photos, max_faces=8, grow=1.0, parse_size=S, resize=stub_resize, components_of=host_components(seen))
    assert seen == [((3, S, S), tuple(fp.FACE_CLASSES), (S // 32) ** 2, 8)]              # one call per chunk, min_area = (parse_size // 32)^2
    assert parser.calls == [((3, 3, S, S), None, tuple(fp.LUT_SEG))]
    by_area = [blobs[0], blobs[2], blobs[1], blobs[3]]                                   # largest first; the 2 x 2 blob has exactly min_area
    assert got[0] == [photo.grow_square_box(scaled(b, 300, 200, S), 300, 200, 1.0) for b in by_area]
    assert got[1] == []                                                                  # no component: an empty list, no error
    assert got[2] == [photo.grow_square_box(scaled((10, 29, 10, 29), 64, 64, S), 64, 64, 1.0)]
    cut = fp.find_faces(parser, photos, max_faces=2, grow=0.5, parse_size=S, resize=stub_resize, components_of=host_components())
    assert cut[0] == [photo.grow_square_box(scaled(b, 300, 200, S), 300, 200, 0.5) for b in by_area[:2]] and cut[1] == []
    big = fp.find_faces(parser, photos, min_area=100, parse_size=S, resize=stub_resize, components_of=host_components())
    assert [len(f) for f in big] == [2, 0, 1]
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError):
            fp.find_faces(parser, photos, max_faces=bad, parse_size=S, resize=stub_resize, components_of=host_components())


def test_find_faces_on_one_blob_is_find_boxes():
    S = 128
    maps = torch.zeros(2, S, S, dtype=torch.uint8)
    maps[0, 40:90, 30:70] = 1; maps[0, 60:64, 40:50] = 7
    maps[1, 5:120, 90:128] = 6
    photos = [torch.zeros(333, 517, 3, dtype=torch.uint8), torch.zeros(1000, 64, 3, dtype=torch.uint8)]
    for grow in (0.0, 1.0):
        faces = fp.find_faces(StubParser(maps), photos, grow=grow, parse_size=S, resize=stub_resize, components_of=host_components())
        boxes = fp.find_boxes(StubParser(maps), photos, grow=grow, parse_size=S, resize=stub_resize, box_of=host_box)
        assert [f[0] for f in faces] == boxes and all(len(f) == 1 for f in faces)


def test_label_components_python_side_checks():
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(mlib.MkdError):
        components.label_components(lab, (1,))                       # a CPU tensor: there is no CPU path
    for bad in (lab.float(), lab[0, 0], 'x'):
        with pytest.raises(ValueError):
            components.label_components(bad, (1,))
    assert components.class_bits((0, 5, 63)) == 1 | 1 << 5 | 1 << 63
    for bad in ((64,), (-1,), (1.5,)):
        with pytest.raises(ValueError):
            components.class_bits(bad)


# ---- the library's argument checks: before anything is enqueued, so they run without a device --------------------------------------
GOOD = dict(labels=0x1000, batch=2, H=40, W=50, classes=2, min_area=1, max_out=16, table=0x2000, count=0x3000, ids=None, scratch=0x4000)
BAD = [dict(batch=0), dict(batch=65536), dict(H=0), dict(W=0), dict(H=-3), dict(H=4097, W=4096), dict(max_out=0), dict(max_out=65),
       dict(min_area=0), dict(min_area=-5), dict(labels=None), dict(table=None), dict(count=None), dict(scratch=None), dict(scratch=0x4010)]


def _call(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.mkd_label_components(C.c_void_p(a['labels']), a['batch'], a['H'], a['W'], C.c_uint64(a['classes']), a['min_area'], a['max_out'],
                                    C.c_void_p(a['table']), C.c_void_p(a['count']), C.c_void_p(a['ids']), C.c_void_p(a['scratch']), None)


@pytest.mark.parametrize('bad', BAD, ids=[str(b) for b in BAD])
def test_bad_arguments_are_refused(bad):
    lib = mlib.load()
    assert _call(lib, **bad) == -1          # MKD_ERR_ARG
    assert lib.mkd_last_error()


def test_scratch_bytes():
    lib = mlib.load()
    for args in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 4097, 4096)):
        assert lib.mkd_label_components_scratch_bytes(*args) == 0
    one = lib.mkd_label_components_scratch_bytes(1, 37, 53)
    assert one % 256 == 0 and one >= 4 * 6 * 37 * 53 and lib.mkd_label_components_scratch_bytes(5, 37, 53) == 5 * one
    assert lib.mkd_label_components_scratch_bytes(1, 4096, 4096) > 0 and lib.mkd_label_components_scratch_bytes(65535, 1, 1) > 0


# ---- transfer_photos(max_faces=...): what it checks before it touches the device ---------------------------------------------------
NET = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64, num_res_blocks=2, in_channels=4,
           use_spatial_transformer=True, legacy=False)


def _model(**kw):
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    return TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=[16, 16, 32, 32, 32, 32, 64])},
                            unet_config={'params': dict(NET, out_channels=4)}, **kw)


def test_transfer_photos_max_faces_checks():
    m = _model()
    p = [torch.zeros(80, 80, 3, dtype=torch.uint8)] * 2
    one, ref = (0, 0, 40, 40), [(0, 0, 80, 80)] * 2
    with pytest.raises(ValueError, match='boxes'):
        m.transfer_photos(p, p, max_faces=2)                                             # no parser and no boxes
    with pytest.raises(ValueError, match='boxes'):
        m.transfer_photos(p, p, [[one], []], None, max_faces=2)                          # ... nor for the references
    with pytest.raises(ValueError, match='list of boxes'):
        m.transfer_photos(p, p, [one, one], ref, max_faces=2)                            # the single-face nesting
    with pytest.raises(ValueError, match='one LIST of boxes per source photo'):
        m.transfer_photos(p, p, [[one]], ref, max_faces=2)
    with pytest.raises(ValueError, match='more than max_faces'):
        m.transfer_photos(p, p, [[one, one, one], []], ref, max_faces=2)
    with pytest.raises(ValueError, match='ref_boxes'):
        m.transfer_photos(p, p, [[one], []], [[(0, 0, 80, 80)], [(0, 0, 80, 80)]], max_faces=2)
    with pytest.raises(ValueError, match='x_T'):
        m.transfer_photos(p, p, [[one, one], [one]], ref, x_T=torch.zeros(2, 4, 8, 8), max_faces=2)      # N = 3
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match='max_faces'):
            m.transfer_photos(p, p, [[one], []], ref, max_faces=bad)
    with pytest.raises(ValueError, match='face_batch'):
        m.transfer_photos(p, p, [[one], []], ref, max_faces=2, face_batch=0)
    with pytest.raises(ValueError, match='only apply with max_faces'):
        m.transfer_photos(p, p, [one, one], ref, return_faces=True)


def test_transfer_photos_without_max_faces_checks_its_boxes():
    """one 4-entry box per photo, source and reference: a wrong count or a 5-entry box (a Frame) is an error, never a partial result"""
    m = _model()
    p = [torch.zeros(80, 80, 3, dtype=torch.uint8)] * 3
    one = (0, 0, 40, 40)
    for src, ref in (([one], [one] * 3), ([one] * 3, [one] * 4), ([one] * 4, [one] * 3), ([one] * 3, [one])):
        with pytest.raises(ValueError, match='3 photos but [14] boxes'):
            m.transfer_photos(p, p, src, ref)
    for bad in ((0, 0, 40, 40, 15.0), photo.Frame(40.0, 40.0, 40.0, 1.0, 0.0), (0, 0, 40)):
        with pytest.raises(ValueError, match='a box is'):
            m.transfer_photos(p, p, [one, bad, one], [one] * 3)
        with pytest.raises(ValueError, match='a box is'):
            m.transfer_photos(p, p, [one] * 3, [one, one, bad])


# ---- boxes files with several faces per image ---------------------------------------------------------------------------------------
def test_read_boxes_multi(tmp_path):
    f = tmp_path / 'boxes.txt'
    f.write_text('# name x0 y0 w h\n\na.png 10 5 64 60\nb.png 1 2 3 4\na.png 70 8 30 30\n\na.png 0 0 9 9\n')
    assert photo.read_boxes_multi(str(f)) == {'a.png': [(10, 5, 64, 60), (70, 8, 30, 30), (0, 0, 9, 9)], 'b.png': [(1, 2, 3, 4)]}
    assert photo.read_boxes(str(f)) == {'a.png': (10, 5, 64, 60), 'b.png': (1, 2, 3, 4)}          # the first line of a name
    for bad in ('a.png 1 2 3\n', 'a.png 1 2 3 x\n'):
        f.write_text(bad)
        with pytest.raises(ValueError):
            photo.read_boxes_multi(str(f))


def test_runs_test_max_faces_flag():
    spec = importlib.util.spec_from_file_location('runs_test_cli_faces', os.path.join(ROOT, 'runs', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.build_parser().parse_args([]).max_faces is None
    assert mod.build_parser().parse_args(['--photos', '--max-faces', '3']).max_faces == 3
