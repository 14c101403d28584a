"""CPU: the guided paste's restatement (tests/photo_guided_ref.py) -- dtypes, positive weight sums and no rint ties on every case the
device tests run, the edge property that is the feature's reason, bytes outside the box -- and what needs no device of the feature
itself: photo.GuidedPaste's range checks and the refusals of the two library entries, which come before anything is enqueued."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import photo_frame_ref as fr
import photo_guided_ref as gr
import photo_ref as pr
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import photo


def test_every_intermediate_keeps_its_dtype_and_the_weight_sum_is_positive():
    """taps asserts the dtype of q, wr, g, sw, sc and u and sw > 0 itself; here it runs on every box and frame case of the device tests"""
    ph = gr.case_photos()
    for S, R, sg, rho, wt in gr.CASES:
        t, s01 = gr.case_samples(S)
        d, yl = gr.model_pixels(t[0], s01[0])
        assert d.dtype == np.float32 and yl.dtype == np.float32
        for T in (np.float32, np.float64):
            q, w = gr.axis_floor(37, S)
            u, sw = gr.taps(d, yl, q[:, None], w[:, None], q[None, :], w[None, :], gr.luma(ph[0][:37, :37]).astype(T), R, sg, T)
            assert u.dtype == T and sw.dtype == T and (sw > 0).all() and np.isfinite(u).all()
        w = gr.case_weights(wt)
        for i, (p, box) in enumerate(gr.case_boxes(S)):
            out = gr.paste(ph[p], box, t[i], s01[i], rho, R, sg, None if w is None else w[i])
            assert out.dtype == np.uint8 and out.shape == ph[p].shape


@pytest.mark.parametrize('k', range(0, len(gr.CASES), 3))
def test_no_frame_case_lies_at_a_tie_of_rint(k):
    """then the frame kernel's bytes are a condition on its arithmetic and not on its last bit"""
    ph = gr.case_photos()
    S, R, sg, rho, wt = gr.CASES[k]
    t, s01 = gr.case_samples(S)
    w = gr.case_weights(wt)
    for i, (p, f) in enumerate(gr.case_frames(S)):
        out, o, inside = gr.paste_frame(ph[p], f, t[i], s01[i], rho, R, sg, None if w is None else w[i])
        assert inside.any() and np.array_equal(out[~inside], ph[p][~inside])
        margin = fr.tie_margin(o[inside])
        assert margin > 1e-9, (i, f, margin)


def test_the_difference_stops_at_the_photos_edge():
    """the construction of the issue: seed 0, S = 32, photo 256^2, box (32, 32, 192, 192), a 60 -> 160 step at x = 132 with +-3 noise,
    +40 levels where the model pixel's luminance exceeds 110 x 256, feather 0.  R = 1, sigma = 8: at most a quarter of the bilinear
    paste's summed absolute change on the dark side (the restatement gives 0 against 1728), and on the bright side a mean change not
    below the bilinear paste's (39.98 against 39.10)"""
    ph, box, t, s01 = gr.edge_case(0)
    assert gr.EDGE_S == 32 and ph.shape == (256, 256, 3) and box == (32, 32, 192, 192) and gr.EDGE_X == 132
    plain_dark, plain_bright = gr.edge_figures(ph, pr.paste(ph, box, t, s01, 0), box)
    guided = gr.paste(ph, box, t, s01, 0, 1, 8.0)
    dark, bright = gr.edge_figures(ph, guided, box)
    print(f'dark side: guided {dark} bilinear {plain_dark}; bright side: guided {bright:.4f} bilinear {plain_bright:.4f}')
    assert plain_dark > 1000 and 38.0 < plain_bright < 40.0                              # the bilinear paste does bleed
    assert 4 * dark <= plain_dark
    assert bright >= plain_bright
    x0, y0, bw, bh = box
    inbox = np.zeros(ph.shape[:2], bool)
    inbox[y0:y0 + bh, x0:x0 + bw] = True
    assert np.array_equal(guided[~inbox], ph[~inbox]) and not np.array_equal(guided[inbox], ph[inbox])


def test_bytes_outside_the_box_and_under_a_zero_weight_stay():
    ph = gr.case_photos()
    S, R, sg, rho = 8, 2, 8.0, 0
    t, s01 = gr.case_samples(S)
    w = gr.case_weights((7, 11))
    changed = 0
    for i, (p, box) in enumerate(gr.case_boxes(S)):
        x0, y0, bw, bh = box
        out = gr.paste(ph[p], box, t[i], s01[i], rho, R, sg, w[i])
        inbox = np.zeros(ph[p].shape[:2], bool)
        inbox[y0:y0 + bh, x0:x0 + bw] = True
        assert np.array_equal(out[~inbox], ph[p][~inbox])
        zero = gr.plane_at_box(w[i], ph[p].shape[0], ph[p].shape[1], box) == 0
        region, was = out[y0:y0 + bh, x0:x0 + bw], ph[p][y0:y0 + bh, x0:x0 + bw]
        assert np.array_equal(region[zero], was[zero])
        changed += int((region[~zero] != was[~zero]).sum())
    assert changed > 1000


def test_radius_zero_and_a_flat_guide_is_the_bilinear_paste_up_to_rounding():
    """R = 0 has the bilinear weights; with sigma = 1e6 the range weight is 1 to within 2^-24, so only the order of the sums differs"""
    ph = gr.case_photos()
    t, s01 = gr.case_samples(16)
    for i, (p, box) in list(enumerate(gr.case_boxes(16)))[:7]:
        a = gr.paste(ph[p], box, np.clip(t[i], -1, 1), s01[i], 0, 0, 1e6).astype(np.int64)
        b = pr.paste(ph[p], box, np.clip(t[i], -1, 1), s01[i], 0).astype(np.int64)
        assert np.abs(a - b).max() <= 1


def test_guided_paste_checks_its_ranges():
    g = photo.GuidedPaste()
    assert (g.radius, g.sigma) == (1, 8.0) and tuple(g) == (1, 8.0) and isinstance(g.sigma, float)
    for R in (0, 1, 2):
        for sg in (0.5, 8, 1e6):
            assert photo.GuidedPaste(R, sg) == (R, float(sg))
    assert photo.GuidedPaste(radius=np.int64(2), sigma=np.float32(3.5)) == (2, 3.5)
    for R in (-1, 3, 1.0, 1.5, '1', None, True):
        with pytest.raises(ValueError, match='radius'):
            photo.GuidedPaste(R, 8.0)
    for sg in (0.25, 0.0, -8.0, 1.0001e6, math.nan, math.inf, -math.inf, None, 'x'):
        with pytest.raises(ValueError, match='sigma'):
            photo.GuidedPaste(1, sg)
    ph = torch.zeros((20, 20, 3), dtype=torch.uint8)
    for fn, region in ((photo.paste_photos, (0, 0, 10, 10)), (photo.paste_frames, (10.0, 10.0, 8.0, 1.0, 0.0)), (photo.paste_regions, (0, 0, 10, 10))):
        with pytest.raises(ValueError, match='GuidedPaste'):                             # before the photos are looked at
            fn([ph], [region], torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), 0, guided=(1, 8.0))
        with pytest.raises(mlib.MkdError, match='HIP device'):                          # there is no CPU path, guided or not
            fn([ph], [region], torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), 0, guided=photo.GuidedPaste())


def test_the_library_entries_refuse_bad_arguments_before_anything_is_enqueued():
    lib = mlib.load()
    S = 16
    FAKE = C.c_void_p(0x1000)
    box = (mlib.PhotoDescC * 1)()
    box[0].pixels, box[0].pitch_bytes, box[0].H, box[0].W = 0x2000, 301, 80, 100
    box[0].x0, box[0].y0, box[0].bw, box[0].bh = 10, 10, 40, 40
    frame = (mlib.PhotoFrameDescC * 1)()
    frame[0].pixels, frame[0].pitch_bytes, frame[0].H, frame[0].W = 0x2000, 301, 80, 100
    frame[0].cx, frame[0].cy, frame[0].side, frame[0].c, frame[0].s = 50.0, 40.0, 30.0, 0.8, 0.6
    for name, d in (('mkd_paste_photo_guided', box), ('mkd_paste_frame_guided', frame)):
        fn = getattr(lib, name)
        call = lambda n=1, t=FAKE, s=FAKE, rho=3, w=None, wh=0, ww=0, R=1, sg=8.0: fn(d, n, S, t, s, rho, w, wh, ww, R, sg, None)
        for kw, word in ((dict(R=3), 'radius'), (dict(R=-1), 'radius'), (dict(sg=0.25), 'sigma'), (dict(sg=math.nan), 'sigma'), (dict(sg=math.inf), 'sigma'),
                         (dict(sg=2e6), 'sigma'), (dict(t=None), ' t '), (dict(s=None), 's01'), (dict(rho=65), 'feather'), (dict(rho=-1), 'feather'),
                         (dict(w=FAKE, wh=0, ww=8), 'wh'), (dict(w=FAKE, wh=8, ww=2049), 'ww'), (dict(n=0), 'descriptors'), (dict(n=17), 'descriptors')):
            assert call(**kw) == -1, (name, kw)
            msg = lib.mkd_last_error().decode()
            assert name in msg and word in msg, (name, kw, msg)
    assert lib.mkd_abi_version() == 1
