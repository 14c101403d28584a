"""CPU: the photo calls' restatement (tests/photo_ref.py) against Pillow's recorded bytes (tests/golden/photo_resize.npz, written by
tools/make_photo_golden.py), the properties of the paste rule, the library's argument checks (they run before anything is enqueued,
so they need no device) and the host side of makeupdiffuse_amd/photo.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import paste_background_ref as pbref
import photo_ref as pr
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import photo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'photo_resize.npz'))
CASES = json.loads(str(GOLD['cases']))


def test_golden_file_covers_the_cases_the_kernel_can_get_wrong():
    assert len(CASES) >= 12 and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'photo_resize.npz')) < 200 * 1024
    ks = [(pr.ksize(c['box'][2], c['size']), pr.ksize(c['box'][3], c['size'])) for c in CASES]
    assert max(max(k) for k in ks) > 7 and min(min(k) for k in ks) == 3                  # shrinking past 3.0 and enlarging
    shapes = [GOLD[f'photo{c["photo"]}'].shape for c in CASES]
    flush = lambda c, s: (c['box'][0] == 0, c['box'][1] == 0, c['box'][0] + c['box'][2] == s[1], c['box'][1] + c['box'][3] == s[0])
    assert all(any(flush(c, s)[i] for c, s in zip(CASES, shapes)) for i in range(4))     # a box on every photo edge
    assert any(c['box'][2] != c['box'][3] for c in CASES)
    assert any(c['box'][2] == c['size'] == s[1] for c, s in zip(CASES, shapes))           # the whole photo with W = S
    assert all(s[0] <= 160 and s[1] <= 203 for s in shapes)


@pytest.mark.parametrize('k', range(len(CASES)))
def test_restatement_gives_pillows_bytes(k):
    c = CASES[k]
    got = pr.crop_resize_u8(GOLD[f'photo{c["photo"]}'], tuple(c['box']), c['size'])
    want = GOLD[f'out{k}']
    assert got.shape == want.shape and np.array_equal(got, want), f'case {c}: {int((got != want).sum())} bytes differ'


def test_coefficient_rows_sum_to_one_and_stay_inside():
    for n, in0, ln, S in ((203, 20, 122, 37), (150, 60, 11, 16), (64, 0, 64, 64), (203, 0, 203, 8), (16384, 0, 16384, 512)):
        b, c = pr.axis_table(n, in0, ln, S)
        assert c.shape[1] == pr.ksize(ln, S) and (c >= 0).all()
        assert (b[:, 0] >= 0).all() and (b[:, 1] <= n).all() and (b[:, 1] - b[:, 0] <= c.shape[1]).all() and (b[:, 1] > b[:, 0]).all()
        assert np.abs(c.sum(1) - (1 << 22)).max() <= c.shape[1]                        # each coefficient is rounded once
    b, c = pr.axis_table(64, 0, 64, 64)
    assert np.array_equal(c[:, 0], np.full(64, 1 << 22)) and not c[:, 1:].any()          # scale 1: the identity, as Pillow's skipped pass


def _crop(photo_u8, box, S):
    return pr.img01(pr.crop_resize_u8(photo_u8, box, S))


PASTE_CASES = [(0, (20, 10, 122, 122), 37), (0, (50, 60, 9, 11), 16), (0, (0, 0, 100, 90), 16), (0, (123, 80, 80, 70), 37),
               (2, (0, 0, 64, 64), 64), (1, (5, 10, 50, 80), 64)]


@pytest.mark.parametrize('rho', [0, 1, 8, 64])
def test_paste_of_the_source_itself_returns_the_photo(rho):
    """t = 2 s01 - 1: d is at most a few ulp of 1 times 255, far below half a grey level, for every box and feather"""
    for pi, box, S in PASTE_CASES:
        ph = GOLD[f'photo{pi}']
        s01 = _crop(ph, box, S)
        t = s01 * np.float32(2.0) - np.float32(1.0)
        assert np.array_equal(pr.paste(ph, box, t, s01, rho), ph), (pi, box, S, rho)


def test_feather_counts_only_sides_inside_the_photo():
    a = pr.feather_alpha(150, 203, (0, 0, 100, 90), 8)                 # left and top lie on the photo's border
    assert a[0, 0] == 1.0 and a[0, 50] == 1.0 and a[89, 50] == np.float32(1) / np.float32(9) and a[40, 99] == np.float32(1) / np.float32(9)
    assert a[40, 95] == np.float32(5) / np.float32(9) and a[40, 50] == 1.0
    assert (pr.feather_alpha(64, 64, (0, 0, 64, 64), 64) == 1.0).all()     # the whole photo: no side fades
    a = pr.feather_alpha(150, 203, (50, 60, 9, 11), 64)                   # a feather larger than the box
    assert a.max() == np.float32(5) / np.float32(65) and a.min() == np.float32(1) / np.float32(65)
    assert (pr.feather_alpha(150, 203, (50, 60, 9, 11), 0) == 1.0).all()


def test_paste_changes_the_box_only_and_clips():
    ph = GOLD['photo2']                                                   # 0 / 255 pixels
    box, S = (7, 9, 41, 33), 16
    s01 = _crop(ph, box, S)
    g = np.random.default_rng(3)
    t = g.uniform(-3.0, 3.0, s01.shape).astype(np.float32)                # beyond +-1: the clip acts
    out = pr.paste(ph, box, t, s01, 1)
    keep = np.ones(ph.shape[:2], bool)
    keep[9:42, 7:48] = False
    assert np.array_equal(out[keep], ph[keep]) and (out[~keep] != ph[~keep]).any()
    assert (out[~keep] == 0).any() and (out[~keep] == 255).any()


def test_a_pasted_background_region_keeps_the_photos_bytes():
    """mkd_paste_background with keep weight 1 puts ((s + 1) / 2) 2 - 1 of the source into the sample; where all four neighbours of a
    photo pixel are such model pixels the photo's bytes come back"""
    ph = GOLD['photo0']
    box, S = (20, 10, 122, 122), 37
    s01 = _crop(ph, box, S)
    g = np.random.default_rng(5)
    t = g.uniform(-1.0, 1.0, s01.shape).astype(np.float32)
    seg = np.zeros((S, S), np.uint8)
    seg[8:30, 6:28] = 1                                                   # the face; 0 is background
    alpha = pbref.alpha_from_labels(seg[None], (0,), 1, 0)
    t2 = pbref.paste(t[None], (s01 * np.float32(2.0) - np.float32(1.0))[None], alpha)[0]
    out = pr.paste(ph, box, t2, s01, 0)
    ya, yb, _ = pr._axis(box[3], S)
    xa, xb, _ = pr._axis(box[2], S)
    bg = seg == 0
    all_bg = bg[ya][:, xa] & bg[ya][:, xb] & bg[yb][:, xa] & bg[yb][:, xb]
    region, was = out[10:132, 20:142], ph[10:132, 20:142]
    assert all_bg.any() and not all_bg.all()
    assert np.array_equal(region[all_bg], was[all_bg])
    assert (region[~all_bg] != was[~all_bg]).mean() > 0.5


# ---- the library's argument checks: before anything is enqueued, so they run without a device ------------------------------------
def _desc(**kw):
    d = dict(pixels=0x1000, pitch_bytes=300, H=80, W=100, x0=10, y0=10, bw=40, bh=40, labels=None)
    d.update(kw)
    arr = (mlib.PhotoDescC * 1)()
    for k, v in d.items():
        setattr(arr[0], k, v)
    return arr


BAD_DESCS = [dict(pixels=None), dict(pitch_bytes=299), dict(H=0), dict(W=16385, pitch_bytes=3 * 16385), dict(bw=0), dict(bh=-1), dict(x0=-1),
             dict(x0=61), dict(y0=41), dict(bw=100, x0=1)]


@pytest.mark.parametrize('bad', BAD_DESCS, ids=[str(b) for b in BAD_DESCS])
def test_bad_descriptors_are_refused_by_every_call(bad):
    lib = mlib.load()
    d = _desc(**bad)
    out, scr = C.c_void_p(0x2000), C.c_void_p(0x4000)
    assert lib.mkd_crop_resize_scratch_bytes(d, 1, 16) == 0
    assert lib.mkd_crop_resize(d, 1, 16, out, None, None, scr, None) == -1
    assert lib.mkd_paste_photo(d, 1, 16, out, out, 8, None) == -1
    assert lib.mkd_last_error()


def test_other_bad_arguments_are_refused():
    lib = mlib.load()
    d, out, scr = _desc(), C.c_void_p(0x2000), C.c_void_p(0x4000)
    for n, S in ((0, 16), (17, 16), (1, 7), (1, 1025)):
        assert lib.mkd_crop_resize(d, n, S, out, None, None, scr, None) == -1
        assert lib.mkd_paste_photo(d, n, S, out, out, 0, None) == -1
        assert lib.mkd_crop_resize_scratch_bytes(d, n, S) == 0
    assert lib.mkd_crop_resize(_desc(bw=40 * 8, bh=8, W=400, pitch_bytes=1200), 1, 8, out, None, None, scr, None) == -1      # > 32 S
    assert lib.mkd_crop_resize(d, 1, 16, None, None, None, scr, None) == -1                # no output
    assert lib.mkd_crop_resize(d, 1, 16, out, None, None, None, None) == -1                # no scratch
    assert lib.mkd_crop_resize(d, 1, 16, out, None, None, C.c_void_p(0x4010), None) == -1  # scratch not 256-byte aligned
    assert lib.mkd_crop_resize(d, 1, 16, out, None, out, scr, None) == -1                  # labels_out without a label map
    assert lib.mkd_crop_resize(None, 1, 16, out, None, None, scr, None) == -1
    for rho in (-1, 65):
        assert lib.mkd_paste_photo(d, 1, 16, out, out, rho, None) == -1
    assert lib.mkd_paste_photo(d, 1, 16, None, out, 0, None) == -1
    for args in ((0, 0, 1, 16), (100, 90, 11, 16), (100, 0, 100, 7), (16385, 0, 64, 64), (100, 0, 100, 2), (100, -1, 10, 16)):
        assert lib.mkd_resize_coeffs(*args, out, out, None) == -1, args
    assert lib.mkd_resize_coeffs(100, 0, 10, 16, None, out, None) == -1


def test_scratch_covers_the_rows_the_vertical_pass_reads():
    lib = mlib.load()
    for H, y0, bh, S in ((150, 10, 122, 37), (150, 0, 150, 16), (150, 60, 11, 16), (97, 0, 97, 16), (16384, 100, 16000, 512), (64, 0, 64, 64)):
        d = _desc(H=H, W=100, y0=y0, bh=bh, x0=0, bw=50)
        nbytes = lib.mkd_crop_resize_scratch_bytes(d, 1, S)
        c = max(1, -(-bh // S))
        lo, hi = max(0, y0 - c - 1), min(H, y0 + bh + c + 1)
        assert nbytes == ((hi - lo) * S * 3 + 255) // 256 * 256
        b, _ = pr.axis_table(H, y0, bh, S)
        assert lo <= b[:, 0].min() and b[:, 1].max() <= hi
    two = (mlib.PhotoDescC * 2)()
    for i, (H, bh) in enumerate(((80, 40), (60, 17))):
        for k, v in dict(pixels=0x1000, pitch_bytes=300, H=H, W=100, x0=0, y0=3, bw=40, bh=bh, labels=None).items():
            setattr(two[i], k, v)
    one = lambda i: lib.mkd_crop_resize_scratch_bytes(C.pointer(two[i]), 1, 16)
    assert lib.mkd_crop_resize_scratch_bytes(two, 2, 16) == one(0) + one(1) and one(0) % 256 == 0


# ---- photo.py on the host ---------------------------------------------------------------------------------------------------------
def test_python_side_validation():
    for box in ((0, 0, 0, 5), (-1, 0, 5, 5), (0, 0, 101, 5), (0, 76, 5, 5), (0, 0, 5.5, 5), (0, 0, 5)):
        with pytest.raises(ValueError):
            photo.check_box(box, 80, 100, 16)
    with pytest.raises(ValueError):
        photo.check_box((0, 0, 300, 10), 80, 400, 8)                  # more than 32 x size
    assert photo.check_box((1.0, 2, 3, 4), 80, 100, 16) == (1, 2, 3, 4)
    ph = torch.zeros(80, 100, 3, dtype=torch.uint8)
    with pytest.raises(mlib.MkdError):
        photo.crop_resize([ph], [(0, 0, 50, 50)], 16)                  # a CPU tensor: there is no CPU path
    with pytest.raises(ValueError):
        photo.crop_resize([ph.float()], [(0, 0, 50, 50)], 16)
    with pytest.raises(ValueError):
        photo.crop_resize([ph[..., :2]], [(0, 0, 50, 50)], 16)
    for size in (7, 1025, 16.5):
        with pytest.raises(ValueError):
            photo.crop_resize([ph], [(0, 0, 50, 50)], size)
    for rho in (-1, 65, 2.5):
        with pytest.raises(ValueError):
            photo.paste_photos([ph], [(0, 0, 50, 50)], torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), rho)
    assert photo.resize_ksize(122, 37) == 9 and photo.resize_ksize(9, 16) == 3 and photo.resize_ksize(64, 64) == 3


@pytest.mark.parametrize('rank', [2, 3])
def test_as_list_takes_a_tensor_a_stacked_batch_and_a_list(rank):
    shape = (2, 3, 4) if rank == 3 else (4, 6)
    one, two = torch.arange(24).reshape(shape), torch.arange(48).reshape((2,) + shape)
    got = [photo.as_list(one, rank), photo.as_list(two, rank), photo.as_list((one, one + 1), rank)]
    assert [len(g) for g in got] == [1, 2, 2] and all(isinstance(g, list) and all(t.dim() == rank for t in g) for g in got)
    assert got[0][0] is one and torch.equal(torch.stack(got[1]), two) and torch.equal(got[2][1], one + 1)


def test_grow_square_box():
    up, down, width = 0.6 / 0.85, 0.2 / 0.85, 0.2 / 0.85
    # a 100 x 60 face (rows 300..399, columns 470..529) in a large photo: grown height 100 (1 + up + down), the longer side
    side = int(round(100 * (1 + up + down)))
    x0, y0, w, h = photo.grow_square_box((300, 399, 470, 529), 1000, 1000, 1.0)
    assert (w, h) == (side, side)
    assert y0 == int(round((300 - up * 100 + 400 + down * 100 - side) / 2.0)) and x0 == int(round((470 + 530 - side) / 2.0))
    assert photo.grow_square_box((300, 399, 470, 529), 1000, 1000, 0.0) == (450, 300, 100, 100)          # no growth: squared only
    # clipped: the square is limited to the shorter side and shifted inside
    x0, y0, w, h = photo.grow_square_box((5, 104, 0, 59), 120, 400, 1.0)
    assert (w, h) == (120, 120) and y0 == 0 and x0 == 0
    x0, y0, w, h = photo.grow_square_box((300, 399, 940, 999), 1000, 1000, 1.0)
    assert x0 + w == 1000 and 0 <= y0 and y0 + h <= 1000
    with pytest.raises(ValueError):
        photo.grow_square_box((2 ** 31 - 1, -1, 2 ** 31 - 1, -1), 100, 100, 1.0)           # the library's "no such label" box
    assert photo.centred_square(150, 203) == (26, 0, 150, 150) and photo.centred_square(97, 64) == (0, 16, 64, 64)


def test_boxes_file_and_photo_dataset(tmp_path):
    from PIL import Image
    g = np.random.default_rng(8)
    sizes = {'non-makeup/s1.png': (90, 120), 'makeup/r1.png': (70, 50)}
    arrays, segs = {}, {}
    for name, (H, W) in sizes.items():
        os.makedirs(tmp_path / 'images' / os.path.dirname(name), exist_ok=True)
        os.makedirs(tmp_path / 'scgan_segs' / os.path.dirname(name), exist_ok=True)
        arrays[name] = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        segs[name] = g.integers(0, 14, (H, W), dtype=np.uint8)
        Image.fromarray(arrays[name]).save(tmp_path / 'images' / name)
        Image.fromarray(segs[name]).save(tmp_path / 'scgan_segs' / name)
    (tmp_path / 'test_0412.txt').write_text('non-makeup/s1.png makeup/r1.png\n')
    (tmp_path / 'boxes.txt').write_text('# name x0 y0 w h\n\nnon-makeup/s1.png 10 5 64 60\n')
    assert photo.read_boxes(str(tmp_path / 'boxes.txt')) == {'non-makeup/s1.png': (10, 5, 64, 60)}
    ds = photo.PhotoPairDataset(str(tmp_path))
    assert len(ds) == 1
    it = ds[0]
    assert it['src_photo'].dtype == torch.uint8 and np.array_equal(it['src_photo'].numpy(), arrays['non-makeup/s1.png'])      # native size
    assert np.array_equal(it['ref_photo'].numpy(), arrays['makeup/r1.png'])
    assert it['src_box'] == (10, 5, 64, 60) and it['ref_box'] == (0, 10, 50, 50)          # boxes.txt, else the centred largest square
    assert np.array_equal(it['src_seg'].numpy(), segs['non-makeup/s1.png']) and tuple(it['ref_seg'].shape) == (70, 50)
    assert it['img_name'] == 's1&r1' and it['txt'] == 'makeup transfer'
    col = photo.collate_photos([it, it])
    assert len(col['src_photo']) == 2 and col['ref_box'] == [(0, 10, 50, 50)] * 2
    (tmp_path / 'boxes.txt').write_text('non-makeup/s1.png 10 5 64\n')
    with pytest.raises(ValueError):
        photo.read_boxes(str(tmp_path / 'boxes.txt'))
    (tmp_path / 'boxes.txt').write_text('non-makeup/s1.png 100 5 64 60\n')
    with pytest.raises(ValueError):
        photo.PhotoPairDataset(str(tmp_path))[0]                            # the box leaves the photo
    os.remove(tmp_path / 'boxes.txt')
    assert photo.PhotoPairDataset(str(tmp_path))[0]['src_box'] == (15, 0, 90, 90)
