"""-m gpu: mkd_paste_photo_guided and mkd_paste_frame_guided against the numpy restatement (tests/photo_guided_ref.py), every output
photo BYTE FOR BYTE.  The cases are photo_guided_ref's (tests/test_photo_guided_host.py runs the restatement alone on them): sixteen
descriptors per call over three photos of differing size with rows 3 W + 1 bytes apart, boxes below, at and above the model size,
1 x 1, one column and one row past the kernel's tile, at every photo corner; frames at roll 0, 17 and -40 degrees and squares that
stick out; every radius and sigma, feather 0 and 64, weight planes with zeros.  Guard bands around every buffer stay intact."""
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

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = 0xA5
GUARD = 64                                   # floats of guard band on both sides of t, s01 and the weight plane


def flat_photo(arr: np.ndarray) -> np.ndarray:
    """the flat host buffer: one sentinel byte, rows 3 W + 1 bytes apart (sentinel padding), and a sentinel tail"""
    H, W = arr.shape[:2]
    flat = np.full(1 + H * (3 * W + 1) + 16, SENTINEL, np.uint8)
    flat[1:1 + H * (3 * W + 1)].reshape(H, 3 * W + 1)[:, :3 * W] = arr.reshape(H, 3 * W)
    return flat


def dev_photo(arr: np.ndarray):
    """-> (device view uint8 [H,W,3] with stride (3 W + 1, 3, 1) one byte into its buffer, the flat device buffer behind it)"""
    H, W = arr.shape[:2]
    buf = torch.from_numpy(flat_photo(arr)).to(DEV)
    return buf.as_strided((H, W, 3), (3 * W + 1, 3, 1), 1), buf


def guarded(a):
    """a float32 host array -> (the device tensor, a contiguous view into a buffer with NaN guard bands; the buffer; its host copy)"""
    if a is None:
        return None, None, None
    host = np.full(a.size + 2 * GUARD, np.nan, np.float32)
    host[GUARD:GUARD + a.size] = a.ravel()
    buf = torch.from_numpy(host).to(DEV)
    return buf[GUARD:GUARD + a.size].view(a.shape), buf, host


def same_bits(buf, host) -> bool:
    return buf is None or np.array_equal(buf.cpu().numpy().view(np.uint32), host.view(np.uint32))


@pytest.fixture(scope='module')
def photos():
    return gr.case_photos()


def run_case(photos, kind, k):
    S, R, sg, rho, wt = gr.CASES[k]
    cases = gr.case_boxes(S) if kind == 'box' else gr.case_frames(S)
    t, s01 = gr.case_samples(S)
    w = gr.case_weights(wt)
    views, bufs = zip(*(dev_photo(photos[p]) for p, _ in cases))
    (dt, bt, ht), (ds, bs, hs), (dw, bw_, hw) = guarded(t), guarded(s01), guarded(w)
    fn = photo.paste_photos if kind == 'box' else photo.paste_frames
    ret = fn(list(views), [r for _, r in cases], dt, ds, rho, weights=dw, guided=photo.GuidedPaste(R, sg))
    assert ret[0] is views[0]
    changed = clipped_lo = clipped_hi = 0
    for i, (p, r) in enumerate(cases):
        wi = None if w is None else w[i]
        if kind == 'box':
            want = gr.paste(photos[p], r, t[i], s01[i], rho, R, sg, wi)
        else:
            want, _, inside = gr.paste_frame(photos[p], r, t[i], s01[i], rho, R, sg, wi)
            assert inside.any() and np.array_equal(want[~inside], photos[p][~inside])
        got = views[i].cpu().numpy()
        assert np.array_equal(got, want), f'{kind} {i} {r} (S {S}, R {R}, sigma {sg}, feather {rho}, plane {wt}): {int((got != want).sum())} bytes differ'
        assert np.array_equal(bufs[i].cpu().numpy(), flat_photo(want)), 'bytes outside the photo rows (pitch padding, leading byte, tail) changed'
        diff = want != photos[p]
        changed += int(diff.sum())
        clipped_lo += int((diff & (want == 0)).sum())
        clipped_hi += int((diff & (want == 255)).sum())
    assert changed > 1000 and clipped_lo > 0 and clipped_hi > 0                          # the pastes did write, and both clips were taken
    assert same_bits(bt, ht) and same_bits(bs, hs) and same_bits(bw_, hw), 't / s01 / the weight plane or their guard bands changed'


@pytest.mark.parametrize('k', range(len(gr.CASES)))
def test_sixteen_mixed_boxes_equal_the_restatement_and_leave_everything_else(photos, k):
    run_case(photos, 'box', k)


@pytest.mark.parametrize('k', range(len(gr.CASES)))
def test_sixteen_mixed_frames_equal_the_restatement_and_leave_everything_else(photos, k):
    run_case(photos, 'frame', k)


def test_single_descriptors_a_zero_plane_and_a_square_that_misses_its_photo(photos):
    S = 8
    t, s01 = gr.case_samples(S)
    dt, ds = torch.from_numpy(t).to(DEV), torch.from_numpy(s01).to(DEV)
    g = photo.GuidedPaste(2, 8.0)
    for i in (4, 10, 14):                                            # n = 1: an interior box, a 1 x 1 box at the corner, one past the tile
        p, box = gr.case_boxes(S)[i]
        view, buf = dev_photo(photos[p])
        photo.paste_photos([view], [box], dt[i:i + 1], ds[i:i + 1], 0, guided=g)
        want = gr.paste(photos[p], box, t[i], s01[i], 0, 2, 8.0)
        assert np.array_equal(buf.cpu().numpy(), flat_photo(want)) and not np.array_equal(want, photos[p])
    p, f = gr.case_frames(S)[5]
    view, buf = dev_photo(photos[p])
    photo.paste_frames([view], [f], dt[5:6], ds[5:6], 8, guided=g)
    want = gr.paste_frame(photos[p], f, t[5], s01[5], 8, 2, 8.0)[0]
    assert np.array_equal(buf.cpu().numpy(), flat_photo(want)) and not np.array_equal(want, photos[p])
    # a weight plane of zeros leaves every byte, in both variants
    zeros = torch.zeros((1, 5, 9), device=DEV)
    for fn, region in ((photo.paste_photos, gr.case_boxes(S)[4][1]), (photo.paste_frames, gr.case_frames(S)[3][1])):
        view, buf = dev_photo(photos[0])
        fn([view], [region], dt[:1], ds[:1], 0, weights=zeros, guided=g)
        assert np.array_equal(buf.cpu().numpy(), flat_photo(photos[0]))
    # no pixel centre inside the square: no launch, no byte changed
    H, W = photos[0].shape[:2]
    assert not fr.inside_mask(H, W, gr.MISS).any()
    view, buf = dev_photo(photos[0])
    photo.paste_frames([view], [gr.MISS], dt[:1], ds[:1], 3, guided=g)
    assert np.array_equal(buf.cpu().numpy(), flat_photo(photos[0]))


def test_regions_send_boxes_and_rolled_frames_to_their_own_entries(photos):
    S, g = 16, photo.GuidedPaste(1, 8.0)
    t, s01 = gr.case_samples(S)
    regions = [gr.case_boxes(S)[4], gr.case_frames(S)[5], gr.case_boxes(S)[14], gr.case_frames(S)[0]]          # (the last: roll 0, a fractional square)
    views, bufs = zip(*(dev_photo(photos[p]) for p, _ in regions))
    photo.paste_regions(list(views), [r for _, r in regions], torch.from_numpy(t[:4]).to(DEV), torch.from_numpy(s01[:4]).to(DEV), 3, guided=g)
    for i, (p, r) in enumerate(regions):
        want = gr.paste(photos[p], r, t[i], s01[i], 3, 1, 8.0) if len(r) == 4 else gr.paste_frame(photos[p], r, t[i], s01[i], 3, 1, 8.0)[0]
        assert np.array_equal(bufs[i].cpu().numpy(), flat_photo(want)), i


def test_the_difference_stops_at_the_photos_edge_on_the_device():
    """tests/test_photo_guided_host.py's edge (S = 32, a x 6 box), on the device's own bytes, box and frame variant"""
    ph, box, t, s01 = gr.edge_case(0)
    dt, ds = torch.from_numpy(t[None]).to(DEV), torch.from_numpy(s01[None]).to(DEV)
    plain = torch.from_numpy(ph).to(DEV)
    photo.paste_photos([plain], [box], dt, ds, 0)
    plain_dark, plain_bright = gr.edge_figures(ph, plain.cpu().numpy(), box)
    assert (plain_dark, round(plain_bright, 2)) == (1728, 39.10)
    view, buf = dev_photo(ph)
    photo.paste_photos([view], [box], dt, ds, 0, guided=photo.GuidedPaste(1, 8.0))
    got = view.cpu().numpy()
    assert np.array_equal(buf.cpu().numpy(), flat_photo(gr.paste(ph, box, t, s01, 0, 1, 8.0)))
    dark, bright = gr.edge_figures(ph, got, box)
    print(f'box: dark {dark} against {plain_dark}, bright {bright:.4f} against {plain_bright:.4f}')
    assert 4 * dark <= plain_dark and bright >= plain_bright
    view, buf = dev_photo(ph)
    f = photo.frame_from_box(box, 0.0)
    photo.paste_frames([view], [tuple(f)], dt, ds, 0, guided=photo.GuidedPaste(1, 8.0))
    assert np.array_equal(buf.cpu().numpy(), flat_photo(gr.paste_frame(ph, tuple(f), t, s01, 0, 1, 8.0)[0]))
    dark, bright = gr.edge_figures(ph, view.cpu().numpy(), box)      # (feather 0: the frame's a = min(e + 0.5, 1) is 1 on every pixel centre)
    print(f'frame: dark {dark}, bright {bright:.4f}')
    assert 4 * dark <= plain_dark and bright >= plain_bright


def test_refused_calls_change_no_byte_and_leave_the_library_usable(photos):
    lib = mlib.load()
    S = 8
    t, s01 = gr.case_samples(S)
    dt, ds = torch.from_numpy(t[:1]).to(DEV), torch.from_numpy(s01[:1]).to(DEV)
    p, box = gr.case_boxes(S)[4]
    _, f = gr.case_frames(S)[0]
    view, buf = dev_photo(photos[p])
    H, W = photos[p].shape[:2]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: C.c_void_p(None if x is None else x.data_ptr())
    db = (mlib.PhotoDescC * 1)()
    db[0].pixels, db[0].pitch_bytes, db[0].H, db[0].W = view.data_ptr(), 3 * W + 1, H, W
    db[0].x0, db[0].y0, db[0].bw, db[0].bh = box
    df = (mlib.PhotoFrameDescC * 1)()
    df[0].pixels, df[0].pitch_bytes, df[0].H, df[0].W = view.data_ptr(), 3 * W + 1, H, W
    df[0].cx, df[0].cy, df[0].side, df[0].c, df[0].s = f
    for name, d in (('mkd_paste_photo_guided', db), ('mkd_paste_frame_guided', df)):
        fn = getattr(lib, name)
        for R, sg, tt, word in ((3, 8.0, dt, 'radius'), (1, 0.25, dt, 'sigma'), (1, math.nan, dt, 'sigma'), (1, math.inf, dt, 'sigma'), (1, 8.0, None, ' t ')):
            assert fn(d, 1, S, P(tt), P(ds), 0, None, 0, 0, R, sg, st) == -1, (name, R, sg)
            msg = lib.mkd_last_error().decode()
            assert name in msg and word in msg, msg
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), flat_photo(photos[p]))
    for bad in (3, -1):
        with pytest.raises(ValueError, match='radius'):
            photo.paste_photos([view], [box], dt, ds, 0, guided=photo.GuidedPaste(bad, 8.0))
    assert np.array_equal(buf.cpu().numpy(), flat_photo(photos[p]))
    # and the next good call of each entry gives the restatement's bytes
    assert lib.mkd_paste_photo_guided(db, 1, S, P(dt), P(ds), 0, None, 0, 0, 1, 8.0, st) == 0
    want = gr.paste(photos[p], box, t[0], s01[0], 0, 1, 8.0)
    assert np.array_equal(buf.cpu().numpy(), flat_photo(want))
    view2, buf2 = dev_photo(photos[p])
    df[0].pixels = view2.data_ptr()
    assert lib.mkd_paste_frame_guided(df, 1, S, P(dt), P(ds), 0, None, 0, 0, 1, 8.0, st) == 0
    assert np.array_equal(buf2.cpu().numpy(), flat_photo(gr.paste_frame(photos[p], f, t[0], s01[0], 0, 1, 8.0)[0]))


def test_none_makes_the_calls_of_today(photos):
    """guided=None: the bytes of the call without the keyword, box and frame, which are photo_ref's / photo_frame_ref's"""
    S = 16
    t, s01 = gr.case_samples(S)
    dt, ds = torch.from_numpy(t[:1]).to(DEV), torch.from_numpy(s01[:1]).to(DEV)
    p, box = gr.case_boxes(S)[4]
    view, buf = dev_photo(photos[p])
    photo.paste_photos([view], [box], dt, ds, 3, guided=None)
    assert np.array_equal(buf.cpu().numpy(), flat_photo(pr.paste(photos[p], box, t[0], s01[0], 3)))
    p, f = gr.case_frames(S)[5]
    view, buf = dev_photo(photos[p])
    photo.paste_frames([view], [f], dt, ds, 3, guided=None)
    assert np.array_equal(buf.cpu().numpy(), flat_photo(fr.paste_frame(photos[p], f, t[0], s01[0], 3)[0]))
