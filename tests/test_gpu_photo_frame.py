"""-m gpu: mkd_crop_frame, mkd_paste_frame and mkd_face_frames against the numpy restatement (tests/photo_frame_ref.py), BYTES and
integers EQUAL.  Photos of at most 96 x 131 with rows an odd number of bytes apart and an unaligned base pointer; the cases (sizes,
rolls, scales, squares that stick out of their photo) are photo_frame_ref's, which tests/test_photo_frame_host.py clears of rint ties
on the CPU: equality is a condition on the kernels and no case is left out."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_frame_ref as fr
from makeupdiffuse_amd import components
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import photo

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = 0xA5
FRAME_RUNS = [(4, None), (1, None), (4, 20)]          # (max_out, min_eye_area), as in tests/test_photo_frame_host.py


def pitch_of(W: int) -> int:
    p = 3 * W + 4
    return p if p % 2 else p + 1                         # odd: no row but the first is aligned to anything


def flat_photo(arr: np.ndarray) -> np.ndarray:
    """the flat host buffer: one sentinel byte, then rows pitch bytes apart with sentinel padding"""
    H, W = arr.shape[:2]
    flat = np.full(1 + H * pitch_of(W), SENTINEL, np.uint8)
    flat[1:].reshape(H, pitch_of(W))[:, :3 * W] = arr.reshape(H, 3 * W)
    return flat


def dev_photo(arr: np.ndarray):
    """-> (device view uint8 [H,W,3] with stride (pitch, 3, 1) one byte into its buffer, the flat device buffer behind it)"""
    H, W = arr.shape[:2]
    buf = torch.from_numpy(flat_photo(arr)).to(DEV)
    return buf.as_strided((H, W, 3), (pitch_of(W), 3, 1), 1), buf


@pytest.fixture(scope='module')
def photos():
    return fr.case_photos(), fr.case_labels()


@pytest.fixture(scope='module')
def crop_refs(photos):
    """{S: [(u8, labels)] of the sixteen frames}, computed once"""
    ph, lab = photos
    return {S: [fr.crop_frame(ph[p], f, S, lab[p])[::2] for p, f in fr.case_frames(S)] for S in fr.CASE_SIZES}


# ---- mkd_crop_frame ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', fr.CASE_SIZES)
def test_sixteen_mixed_crops_equal_the_restatement(photos, crop_refs, S):
    ph, lab = photos
    cases = fr.case_frames(S)
    views = [dev_photo(ph[p])[0] for p, _ in cases]
    got = photo.crop_frames(views, [f for _, f in cases], S, labels=[torch.from_numpy(lab[p]).to(DEV) for p, _ in cases], want_u8=True)
    u8, labels, img = got.u8.cpu().numpy(), got.labels.cpu().numpy(), got.img01.cpu().numpy()
    for k, (want_u8, want_lab) in enumerate(crop_refs[S]):
        assert np.array_equal(u8[k], want_u8), f'frame {k} {cases[k]}: {int((u8[k] != want_u8).sum())} bytes differ'
        assert np.array_equal(labels[k], want_lab), f'frame {k}: labels'
        assert np.array_equal(img[k], fr.img01(want_u8)), f'frame {k}: img01'


@pytest.mark.parametrize('S', fr.CASE_SIZES)
def test_single_crops_with_outputs_switched_off(photos, crop_refs, S):
    """n = 1: img01 alone (no labels, no u8), and the library called directly with u8_out alone (img01 NULL)"""
    ph, lab = photos
    lib = mlib.load()
    for p, f in fr.extra_frames(S):
        want = fr.crop_frame(ph[p], f, S)[0]
        view, _ = dev_photo(ph[p])
        got = photo.crop_frames([view], [f], S)
        assert got.labels is None and got.u8 is None
        assert np.array_equal(got.img01[0].cpu().numpy(), fr.img01(want)), (p, f)
        d = (mlib.PhotoFrameDescC * 1)()
        d[0].pixels, d[0].pitch_bytes, d[0].H, d[0].W = view.data_ptr(), int(view.stride(0)), view.shape[0], view.shape[1]
        d[0].cx, d[0].cy, d[0].side, d[0].c, d[0].s = f
        u8 = torch.full((S, S, 3), SENTINEL, device=DEV, dtype=torch.uint8)
        assert lib.mkd_crop_frame(d, 1, S, None, C.c_void_p(u8.data_ptr()), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert np.array_equal(u8.cpu().numpy(), want), (p, f)
    k = 3                                                    # one of the sixteen on its own: the batch changes nothing
    p, f = fr.case_frames(S)[k]
    got = photo.crop_frames([dev_photo(ph[p])[0]], [f], S, labels=[torch.from_numpy(lab[p]).to(DEV)], want_u8=True)
    assert np.array_equal(got.u8[0].cpu().numpy(), crop_refs[S][k][0]) and np.array_equal(got.labels[0].cpu().numpy(), crop_refs[S][k][1])


# ---- mkd_paste_frame -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(fr.PASTE_CASES)))
def test_sixteen_mixed_pastes_equal_the_restatement_and_leave_everything_else(photos, k):
    ph, _ = photos
    S, rho, wt = fr.PASTE_CASES[k]
    cases = fr.case_frames(S)
    t, s01 = fr.case_samples(S)
    w = fr.case_weights(wt)
    views, bufs = zip(*(dev_photo(ph[p]) for p, _ in cases))
    ret = photo.paste_frames(list(views), [f for _, f in cases], torch.from_numpy(t).to(DEV), torch.from_numpy(s01).to(DEV), rho,
                             weights=None if w is None else torch.from_numpy(w).to(DEV))
    assert ret[0] is views[0]
    for i, (p, f) in enumerate(cases):
        want, _, inside = fr.paste_frame(ph[p], f, t[i], s01[i], rho, None if w is None else w[i])
        assert inside.any() and np.array_equal(want[~inside], ph[p][~inside])
        got = views[i].cpu().numpy()
        assert np.array_equal(got, want), f'frame {i} {f}: {int((got != want).sum())} bytes differ'
        assert np.array_equal(bufs[i].cpu().numpy(), flat_photo(want)), 'bytes outside the photo rows (pitch padding, leading byte) changed'


def test_single_paste_and_a_square_that_misses_its_photo(photos):
    ph, _ = photos
    S = 16
    t, s01 = fr.case_samples(S)
    p, f = fr.case_frames(S)[2]
    view, buf = dev_photo(ph[p])
    photo.paste_frames([view], [f], torch.from_numpy(t[2:3]).to(DEV), torch.from_numpy(s01[2:3]).to(DEV), 8)
    want = fr.paste_frame(ph[p], f, t[2], s01[2], 8)[0]
    assert np.array_equal(buf.cpu().numpy(), flat_photo(want)) and not np.array_equal(want, ph[p])
    H, W = ph[0].shape[:2]
    view, buf = dev_photo(ph[0])
    miss = fr.frame(-9.9, -9.9, 10.0, 45.0)                  # within its side of the photo, but no pixel centre inside: nothing to write
    assert not fr.inside_mask(H, W, miss).any()
    photo.paste_frames([view], [miss], torch.from_numpy(t[:1]).to(DEV), torch.from_numpy(s01[:1]).to(DEV), 3)
    assert np.array_equal(buf.cpu().numpy(), flat_photo(ph[0]))


def test_refused_calls_write_nothing(photos):
    ph, lab = photos
    lib = mlib.load()
    S = 16
    view, buf = dev_photo(ph[0])
    H, W = ph[0].shape[:2]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(None if t is None else t.data_ptr())

    def desc(**kw):
        d = (mlib.PhotoFrameDescC * 1)()
        v = dict(pixels=view.data_ptr(), pitch_bytes=int(view.stride(0)), H=H, W=W, cx=60.0, cy=40.0, side=30.0, c=0.8, s=0.6, labels=None)
        v.update(kw)
        for k, x in v.items():
            setattr(d[0], k, x)
        return d
    img = torch.full((3, S, S * 4), SENTINEL, device=DEV, dtype=torch.uint8)
    u8 = torch.full((S, S, 3), SENTINEL, device=DEV, dtype=torch.uint8)
    lo = torch.full((S, S), SENTINEL, device=DEV, dtype=torch.uint8)
    dt, ds = torch.zeros((1, 3, S, S), device=DEV), torch.ones((1, 3, S, S), device=DEV)
    w = torch.ones((1, 8, 8), device=DEV)
    bad_descs = [dict(pixels=None), dict(H=0), dict(W=16385), dict(pitch_bytes=3 * W - 1), dict(cx=float('nan')), dict(side=0.0), dict(side=32.0 * S + 1),
                 dict(c=0.8, s=0.61), dict(cx=-30.5), dict(cy=H + 30.5)]
    for bad in bad_descs:
        assert lib.mkd_crop_frame(desc(**bad), 1, S, P(img), P(u8), None, st) == -1 and lib.mkd_last_error(), bad
        assert lib.mkd_paste_frame(desc(**bad), 1, S, P(dt), P(ds), 3, None, 0, 0, st) == -1 and lib.mkd_last_error(), bad
    for n, s_, lab_out in ((0, S, None), (17, S, None), (1, 7, None), (1, 1025, None), (1, S, lo)):                # labels_out without a label map
        assert lib.mkd_crop_frame(desc(), n, s_, P(img), P(u8), P(lab_out), st) == -1 and lib.mkd_last_error(), (n, s_)
    assert lib.mkd_crop_frame(desc(), 1, S, None, None, None, st) == -1
    for t_, s_, rho, wp, wh, ww in ((None, ds, 3, None, 0, 0), (dt, None, 3, None, 0, 0), (dt, ds, -1, None, 0, 0), (dt, ds, 65, None, 0, 0),
                                    (dt, ds, 3, w, 0, 8), (dt, ds, 3, w, 8, 2049)):
        assert lib.mkd_paste_frame(desc(), 1, S, P(t_), P(s_), rho, P(wp), wh, ww, st) == -1 and lib.mkd_last_error(), (rho, wh, ww)
    torch.cuda.synchronize()
    assert (img == SENTINEL).all() and (u8 == SENTINEL).all() and (lo == SENTINEL).all()
    assert np.array_equal(buf.cpu().numpy(), flat_photo(ph[0]))
    for bad in (w[0], w.double(), torch.ones((2, 8, 8), device=DEV), torch.ones((1, 8, 2049), device=DEV)):
        with pytest.raises(ValueError, match='weights'):
            photo.paste_frames([view], [(60.0, 40.0, 30.0, 0.8, 0.6)], dt, ds, 3, weights=bad)
    # mkd_face_frames
    B, Sf, K = 2, 16, 4
    labels = torch.zeros((B, Sf, Sf), device=DEV, dtype=torch.uint8)
    ids = torch.full((B, Sf, Sf), -1, device=DEV, dtype=torch.int32)
    table = torch.from_numpy(np.tile(np.array(components.FILL_ROW, np.int32), (B, K, 1))).to(DEV)
    frames = torch.full((B, K, 48), SENTINEL, device=DEV, dtype=torch.uint8)
    scratch = torch.full((int(lib.mkd_face_frames_scratch_bytes(B, K)) + 512,), SENTINEL, device=DEV, dtype=torch.uint8)
    base = (scratch.data_ptr() + 255) & ~255
    hw = (C.c_int32 * 4)(100, 200, 300, 400)
    good = dict(labels=P(labels), ids=P(ids), table=P(table), batch=B, S=Sf, max_out=K, hw=hw, area=1, frames=P(frames), scratch=C.c_void_p(base))
    for bad in (dict(batch=0), dict(batch=17), dict(S=0), dict(S=4097), dict(max_out=0), dict(max_out=65), dict(area=0), dict(labels=None), dict(ids=None),
                dict(table=None), dict(hw=None), dict(frames=None), dict(scratch=None), dict(scratch=C.c_void_p(base + 16)),
                dict(hw=(C.c_int32 * 4)(100, 200, 0, 400)), dict(hw=(C.c_int32 * 4)(100, 16385, 300, 400))):
        a = dict(good, **bad)
        rc = lib.mkd_face_frames(a['labels'], a['ids'], a['table'], a['batch'], a['S'], a['max_out'], a['hw'], C.c_uint64(16), C.c_uint64(32), a['area'],
                                 a['frames'], a['scratch'], st)
        assert rc == -1 and lib.mkd_last_error(), bad
    torch.cuda.synchronize()
    assert (frames == SENTINEL).all() and (scratch == SENTINEL).all()


# ---- mkd_face_frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [16, 64])
@pytest.mark.parametrize('run', range(len(FRAME_RUNS)))
def test_face_frames_equal_the_integer_restatement(S, run):
    max_out, area = FRAME_RUNS[run]
    lab, hw = fr.frames_maps(S)
    dl = torch.from_numpy(lab).to(DEV)
    table, count, ids = components.label_components(dl, fp.FACE_CLASSES, min_area=1, max_out=max_out, want_ids=True)
    assert count.cpu().tolist() == [2, 0, 1, 2, 3]                                 # max_out = 1 cuts components off
    got = components.face_frames(dl, ids, table, hw, min_eye_area=area)
    assert got.dtype == torch.int64 and tuple(got.shape) == (5, max_out, 8) and got.device.type == 'cuda'
    want = fr.face_frames(lab, ids.cpu().numpy(), table.cpu().numpy(), hw, min_eye_area=area)
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:8]
    again = components.face_frames(dl, ids, table, hw, min_eye_area=area)
    assert torch.equal(again, got)                                                 # integers: the same bytes on every run


def test_face_frames_splits_large_batches_and_checks_its_inputs():
    S = 64
    lab, hw = fr.frames_maps(S)
    big = torch.from_numpy(np.concatenate([lab] * 4)[:18]).to(DEV)                 # 18 images: two library calls
    hw18 = (hw * 4)[:18]
    table, _, ids = components.label_components(big, fp.FACE_CLASSES, min_area=1, max_out=3, want_ids=True)
    got = components.face_frames(big, ids, table, hw18).cpu().numpy()
    want = fr.face_frames(big.cpu().numpy(), ids.cpu().numpy(), table.cpu().numpy(), hw18)
    assert np.array_equal(got, want)
    for bad_hw in (hw18[:17], [(0, 5)] * 18, [(5, 16385)] * 18):
        with pytest.raises(ValueError, match='photo_hw'):
            components.face_frames(big, ids, table, bad_hw)
    with pytest.raises(ValueError, match='min_eye_area'):
        components.face_frames(big, ids, table, hw18, min_eye_area=0)
