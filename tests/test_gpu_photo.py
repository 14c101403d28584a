"""-m gpu: mkd_crop_resize, mkd_resize_coeffs and mkd_paste_photo bit for bit against Pillow's recorded bytes
(tests/golden/photo_resize.npz) and the numpy restatement (tests/photo_ref.py).  No tolerance anywhere.  Shapes are sized to the
kernels' blocks (32 output columns / 8 output rows / 64 photo rows per block, 64 x 16 paste tiles), not to real photos; every photo
sits in a buffer with pitch 3 W + 5 behind a base pointer that is off by one byte."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import photo_ref as pr
from gpu_util import DEV
from makeupdiffuse_amd import photo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'photo_resize.npz'))
CASES = json.loads(str(GOLD['cases']))
SENTINEL = 0xA5


def flat_photo(arr: np.ndarray):
    """-> (the flat host buffer: one sentinel byte, then rows 3 W + 5 bytes apart; pitch)"""
    H, W = arr.shape[:2]
    pitch = 3 * W + 5
    flat = np.full(1 + H * pitch, SENTINEL, np.uint8)
    rows = flat[1:].reshape(H, pitch)
    rows[:, :3 * W] = arr.reshape(H, 3 * W)
    return flat, pitch


def dev_photo(arr: np.ndarray):
    """-> (device view uint8 [H,W,3] with stride (3 W + 5, 3, 1) and an odd base address, the flat device buffer behind it)"""
    flat, pitch = flat_photo(arr)
    buf = torch.from_numpy(flat).to(DEV)
    view = buf.as_strided((arr.shape[0], arr.shape[1], 3), (pitch, 3, 1), 1)
    assert view.data_ptr() % 2 == 1 and pitch % 4 != 0
    return view, buf


@functools.lru_cache(maxsize=None)
def ref_crop(pi: int, box, S: int):
    u8 = pr.crop_resize_u8(GOLD[f'photo{pi}'], box, S)
    return u8, pr.img01(u8)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.mark.parametrize('S', [16, 37, 64])
def test_crop_resize_gives_pillows_bytes_for_a_mixed_batch(S):
    ks = [k for k, c in enumerate(CASES) if c['size'] == S]
    assert len(ks) >= 3 and len({GOLD[f'photo{CASES[k]["photo"]}'].shape for k in ks}) >= 2          # photos of different sizes
    photos = [dev_photo(GOLD[f'photo{CASES[k]["photo"]}'])[0] for k in ks]
    boxes = [tuple(CASES[k]['box']) for k in ks]
    out = photo.crop_resize(photos, boxes, S, want_u8=True)
    u8, f = out.u8.cpu().numpy(), out.img01.cpu().numpy()
    assert out.labels is None and u8.shape == (len(ks), S, S, 3) and f.shape == (len(ks), 3, S, S) and f.dtype == np.float32
    for i, k in enumerate(ks):
        want = GOLD[f'out{k}']
        assert np.array_equal(u8[i], want), f'case {CASES[k]}: {int((u8[i] != want).sum())} bytes differ from Pillow'
        assert np.array_equal(bits(f[i]), bits(pr.img01(want))), f'case {CASES[k]}: img01 is not float(u8) / 255'
        assert np.array_equal(want, ref_crop(CASES[k]['photo'], boxes[i], S)[0])


def test_crop_resize_batch_of_16_and_the_split_above_it_with_labels():
    ks = [k for k, c in enumerate(CASES) if c['size'] == 16]
    g = np.random.default_rng(12)
    labels_np = {pi: g.integers(0, 256, GOLD[f'photo{pi}'].shape[:2], dtype=np.uint8) for pi in range(4)}       # classes >= 64 too
    assert all((l >= 64).any() for l in labels_np.values())
    for n in (16, 19):
        pick = [ks[i % len(ks)] for i in range(n)]
        photos = [dev_photo(GOLD[f'photo{CASES[k]["photo"]}'])[0] for k in pick]
        labels = [torch.from_numpy(labels_np[CASES[k]['photo']]).to(DEV) for k in pick]
        boxes = [tuple(CASES[k]['box']) for k in pick]
        out = photo.crop_resize(photos, boxes, 16, labels=labels, want_u8=True)
        u8, lab, f = out.u8.cpu().numpy(), out.labels.cpu().numpy(), out.img01.cpu().numpy()
        for i, k in enumerate(pick):
            assert np.array_equal(u8[i], GOLD[f'out{k}']), (n, i, CASES[k])
            assert np.array_equal(bits(f[i]), bits(pr.img01(GOLD[f'out{k}']))), (n, i)
            assert np.array_equal(lab[i], pr.crop_labels(labels_np[CASES[k]['photo']], boxes[i], 16)), (n, i, CASES[k])


def test_img01_alone_and_contiguous_photos_give_the_same_bytes():
    k = 0
    c = CASES[k]
    ph = torch.from_numpy(GOLD[f'photo{c["photo"]}']).to(DEV)              # contiguous, aligned
    out = photo.crop_resize(ph[None], [tuple(c['box'])], c['size'])        # one [B,H,W,3] tensor, no u8, no labels
    assert out.u8 is None and out.labels is None
    assert np.array_equal(bits(out.img01[0].cpu().numpy()), bits(pr.img01(GOLD[f'out{k}'])))


AXES = [(203, 20, 122, 37), (150, 60, 11, 16), (203, 0, 100, 16), (203, 123, 80, 37), (64, 0, 64, 64), (150, 0, 150, 16), (200, 3, 190, 37),
        (97, 10, 80, 64), (203, 0, 203, 64), (1000, 0, 1000, 32)]


@pytest.mark.parametrize('n,in0,length,S', AXES)
def test_resize_coeffs_equal_the_restatements_tables(n, in0, length, S):
    bounds, coef = photo.resize_coeffs(n, in0, length, S, device=DEV)
    wb, wc = pr.axis_table(n, in0, length, S)
    assert tuple(coef.shape) == wc.shape
    assert np.array_equal(bounds.cpu().numpy(), wb), 'bounds differ'
    assert np.array_equal(coef.cpu().numpy(), wc), f'{int((coef.cpu().numpy() != wc).sum())} coefficients differ'


PASTE_BATCHES = {16: [(0, (50, 60, 9, 11)), (0, (0, 0, 100, 90)), (2, (7, 9, 41, 33))],            # the first box is smaller than every feather > 4
                 37: [(0, (20, 10, 122, 122)), (0, (123, 80, 80, 70)), (3, (3, 2, 190, 36))],
                 64: [(2, (0, 0, 64, 64)), (1, (5, 10, 50, 80))]}


@functools.lru_cache(maxsize=None)
def paste_inputs(S: int):
    g = np.random.default_rng(100 + S)
    entries = PASTE_BATCHES[S]
    s01 = np.stack([ref_crop(pi, box, S)[1] for pi, box in entries])
    t = g.uniform(-3.0, 3.0, s01.shape).astype(np.float32)                # beyond +-1: the clip to 0..255 acts
    return s01, t


@pytest.mark.parametrize('rho', [0, 1, 8, 64])
@pytest.mark.parametrize('S', [16, 37, 64])
def test_paste_photo_equals_the_restatement_and_leaves_everything_else(S, rho):
    entries = PASTE_BATCHES[S]
    s01, t = paste_inputs(S)
    views, bufs = zip(*(dev_photo(GOLD[f'photo{pi}']) for pi, _ in entries))
    ret = photo.paste_photos(list(views), [b for _, b in entries], torch.from_numpy(t).to(DEV), torch.from_numpy(s01).to(DEV), rho)
    assert ret[0] is views[0]
    low = high = False
    for i, (pi, box) in enumerate(entries):
        ph = GOLD[f'photo{pi}']
        want = pr.paste(ph, box, t[i], s01[i], rho)
        x0, y0, bw, bh = box
        inside = np.zeros(ph.shape[:2], bool)
        inside[y0:y0 + bh, x0:x0 + bw] = True
        assert np.array_equal(want[~inside], ph[~inside])
        got = views[i].cpu().numpy()
        assert np.array_equal(got, want), f'S {S} rho {rho} entry {i}: {int((got != want).sum())} bytes differ'
        assert np.array_equal(bufs[i].cpu().numpy(), flat_photo(want)[0]), 'bytes outside the photo rows (pitch padding, leading byte) changed'
        low, high = low or bool((want[inside] == 0).any()), high or bool((want[inside] == 255).any())
    assert low and high                                                   # (of the restatement: the inputs make the clip act)


@pytest.mark.parametrize('rho', [0, 8, 64])
def test_paste_of_the_source_itself_leaves_the_photo(rho):
    for S, entries in PASTE_BATCHES.items():
        views, bufs = zip(*(dev_photo(GOLD[f'photo{pi}']) for pi, _ in entries))
        boxes = [b for _, b in entries]
        s01 = photo.crop_resize(list(views), boxes, S).img01               # the device's own img01
        assert np.array_equal(bits(s01.cpu().numpy()), bits(paste_inputs(S)[0]))
        photo.paste_photos(list(views), boxes, s01 * 2.0 - 1.0, s01, rho)
        for (pi, _), buf in zip(entries, bufs):
            assert np.array_equal(buf.cpu().numpy(), flat_photo(GOLD[f'photo{pi}'])[0]), (S, rho, pi)


def test_engine_free_calls_refuse_what_the_library_refuses():
    ph = dev_photo(GOLD['photo0'])[0]
    with pytest.raises(ValueError):
        photo.crop_resize([ph], [(0, 0, 204, 10)], 16)
    with pytest.raises(ValueError):
        photo.paste_photos([ph.permute(1, 0, 2)], [(0, 0, 10, 10)], torch.zeros(1, 3, 16, 16, device=DEV), torch.zeros(1, 3, 16, 16, device=DEV), 0)
    with pytest.raises(ValueError):
        photo.crop_resize([ph], [(0, 0, 50, 50)], 16, labels=[torch.zeros(10, 10, dtype=torch.uint8, device=DEV)])


def test_square_box_from_labels_uses_the_devices_bounding_box():
    seg = torch.zeros(300, 400, dtype=torch.uint8)
    seg[100:200, 170:230] = 1
    seg[120:125, 180:190] = 4
    seg[10:20, 10:20] = 12                                                 # hair is not a face class
    boxes = photo.square_box_from_labels([seg.to(DEV)], classes=(1, 4), grow=1.0)
    assert boxes == [photo.grow_square_box((100, 199, 170, 229), 300, 400, 1.0)]
    x0, y0, w, h = boxes[0]
    assert w == h and 0 <= x0 and 0 <= y0 and x0 + w <= 400 and y0 + h <= 300
    with pytest.raises(ValueError):
        photo.square_box_from_labels(seg.to(DEV), classes=(7,), grow=1.0)
