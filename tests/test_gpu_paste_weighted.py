"""-m gpu: mkd_paste_photo_weighted against the numpy restatement (tests/owner_ref.py paste_weighted, built on tests/photo_ref.py),
byte for byte: a 61 x 47 photo with rows an odd number of bytes apart, one box inside it and one on its border, random weights in
[0, 1] on a grid coarser (16 x 16) and finer (64 x 64) than the photo; and the two ends of the weight: 1 everywhere is mkd_paste_photo,
0 everywhere leaves the photo."""
import ctypes as C

import numpy as np
import pytest
import torch

import owner_ref as orf
import photo_ref as pr
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import photo

pytestmark = pytest.mark.gpu

DEV = 'cuda'
H, W, S = 61, 47, 16
PITCH = 3 * W + 4                                    # 145 bytes: odd, so no row but the first is aligned to anything
BOXES = [(9, 12, 30, 35), (17, 0, 30, 61)]          # inside; on the top, bottom and right border (x0 + bw = W)
SENTINEL = 0xA5


def flat_photo(arr: np.ndarray) -> np.ndarray:
    """the flat host buffer: one sentinel byte, then rows PITCH bytes apart with sentinel padding"""
    flat = np.full(1 + H * PITCH, SENTINEL, np.uint8)
    flat[1:].reshape(H, PITCH)[:, :3 * W] = arr.reshape(H, 3 * W)
    return flat


def dev_photo(arr: np.ndarray):
    """-> (device view uint8 [H,W,3] with stride (PITCH, 3, 1) one byte into its buffer, the flat device buffer behind it)"""
    buf = torch.from_numpy(flat_photo(arr)).to(DEV)
    return buf.as_strided((H, W, 3), (PITCH, 3, 1), 1), buf


@pytest.fixture(scope='module')
def inputs():
    g = np.random.default_rng(6147)
    ph = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    s01 = g.random((len(BOXES), 3, S, S)).astype(np.float32)
    t = g.uniform(-3.0, 3.0, s01.shape).astype(np.float32)               # beyond +-1: the clip to 0..255 acts
    return ph, s01, t


def run(ph, s01, t, rho, w):
    """both boxes in one call, each into a copy of the photo of its own -> [(bytes of the photo, the flat buffer behind it)]"""
    views, bufs = zip(*(dev_photo(ph) for _ in BOXES))
    ret = photo.paste_photos(list(views), BOXES, torch.from_numpy(t).to(DEV), torch.from_numpy(s01).to(DEV), rho,
                             weights=None if w is None else torch.from_numpy(w).to(DEV))
    assert ret[0] is views[0]
    return [(v.cpu().numpy(), b.cpu().numpy()) for v, b in zip(views, bufs)]


@pytest.mark.parametrize('rho', [0, 3])
@pytest.mark.parametrize('wh,ww', [(16, 16), (64, 64), (1, 1), (7, 64)])
def test_weighted_paste_equals_the_restatement_and_leaves_everything_else(inputs, wh, ww, rho):
    ph, s01, t = inputs
    w = np.random.default_rng(wh * 100 + ww).random((len(BOXES), wh, ww)).astype(np.float32)
    for i, (got, flat) in enumerate(run(ph, s01, t, rho, w)):
        want = orf.paste_weighted(ph, BOXES[i], t[i], s01[i], rho, w[i])
        x0, y0, bw, bh = BOXES[i]
        inside = np.zeros((H, W), bool)
        inside[y0:y0 + bh, x0:x0 + bw] = True
        assert np.array_equal(want[~inside], ph[~inside]) and (want[inside] != ph[inside]).mean() > 0.3
        assert np.array_equal(got, want), f'box {i}: {int((got != want).sum())} bytes differ'
        assert np.array_equal(flat, flat_photo(want)), 'bytes outside the photo rows (pitch padding, leading byte) changed'


def test_weight_one_is_the_plain_paste_and_weight_zero_leaves_the_photo(inputs):
    ph, s01, t = inputs
    plain = run(ph, s01, t, 3, None)
    ones = run(ph, s01, t, 3, np.ones((len(BOXES), 16, 16), np.float32))
    zeros = run(ph, s01, t, 3, np.zeros((len(BOXES), 64, 64), np.float32))
    for i in range(len(BOXES)):
        assert np.array_equal(plain[i][0], pr.paste(ph, BOXES[i], t[i], s01[i], 3)) and not np.array_equal(plain[i][0], ph)
        assert np.array_equal(ones[i][1], plain[i][1])
        assert np.array_equal(zeros[i][1], flat_photo(ph))


def test_a_weight_plane_belongs_to_its_descriptor(inputs):
    """plane 0 all one, plane 1 all zero: the first photo gets the plain paste, the second stays"""
    ph, s01, t = inputs
    w = np.stack([np.ones((16, 16), np.float32), np.zeros((16, 16), np.float32)])
    got = run(ph, s01, t, 0, w)
    assert np.array_equal(got[0][0], pr.paste(ph, BOXES[0], t[0], s01[0], 0)) and np.array_equal(got[1][0], ph)


def test_refused_calls_write_nothing(inputs):
    ph, s01, t = inputs
    lib = mlib.load()
    view, buf = dev_photo(ph)
    d = (mlib.PhotoDescC * 1)()
    d[0].pixels, d[0].pitch_bytes, d[0].H, d[0].W = view.data_ptr(), int(view.stride(0)), H, W
    d[0].x0, d[0].y0, d[0].bw, d[0].bh = BOXES[0]
    dt, ds = torch.from_numpy(t[:1]).to(DEV), torch.from_numpy(s01[:1]).to(DEV)
    w = torch.ones((1, 16, 16), device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for wp, wh, ww in ((None, 16, 16), (w.data_ptr(), 16, 2049), (w.data_ptr(), 2049, 16), (w.data_ptr(), 0, 16), (w.data_ptr(), 16, 0)):
        rc = lib.mkd_paste_photo_weighted(d, 1, S, C.c_void_p(dt.data_ptr()), C.c_void_p(ds.data_ptr()), 3, C.c_void_p(wp), wh, ww, st)
        assert rc == -1 and lib.mkd_last_error(), (wp, wh, ww)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), flat_photo(ph))
    for bad in (w[0], w.double(), torch.ones((2, 16, 16), device=DEV), torch.ones((1, 16, 2049), device=DEV)):
        with pytest.raises(ValueError, match='weights'):
            photo.paste_photos([view], BOXES[:1], dt, ds, 3, weights=bad)
