"""CPU: the landmark-warped term of the teacher.  The host solve (teacher.tps_coefficients), the definition (tests/teacher_warp_ref.py, the
restatement mkd_pgt_warp is held to on the device) on cases with an analytic answer, and the refusals of the C entry, the model, the
dataset and the command line that need no device."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import teacher_warp_ref as wr
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import teacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def distinct_points(rng, K, H, W):
    flat = rng.choice(H * W, K, replace=False)
    return np.stack([flat // W, flat % W], 1).astype(np.float64)


def at_points(q, pts):
    """q [2, H, W] at integer points [K, 2] -> [K, 2]"""
    y, x = pts[:, 0].astype(int), pts[:, 1].astype(int)
    return np.stack([q[0, y, x], q[1, y, x]], 1)


# ---- 1. the host solve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,size', [(3, 8), (20, 32), (68, 64), (68, 256)])
def test_spline_interpolates_every_landmark(K, size):
    rng = np.random.RandomState(K + size)
    src = np.stack([distinct_points(rng, K, size, size) for _ in range(2)])
    ref = src + rng.uniform(-size / 16, size / 16, src.shape)
    ctrl, coef, kcount = teacher.tps_coefficients(src, ref, max_ctrl=K + 5)
    assert ctrl.dtype == np.float64 and coef.dtype == np.float64 and kcount.dtype == np.int32
    assert ctrl.shape == (2, K + 5, 2) and coef.shape == (2, 2, K + 8) and kcount.tolist() == [K, K]
    assert np.array_equal(ctrl[:, :K], src) and not ctrl[:, K:].any() and not coef[:, :, K:K + 5].any()
    q = wr.spline_map(ctrl, coef, kcount, size, size)
    for b in range(2):
        assert np.abs(at_points(q[b], src[b]) - ref[b]).max() <= 1e-6
    # the tests' own solve agrees, and tensors are taken like arrays
    c1, f1 = wr.solve(src[0], ref[0], K + 5)
    assert np.array_equal(c1, ctrl[0]) and np.allclose(f1, coef[0], rtol=0, atol=1e-9 * max(1.0, np.abs(f1).max()))
    t = teacher.tps_coefficients(torch.from_numpy(src), torch.from_numpy(ref).float(), max_ctrl=K + 5)
    assert np.array_equal(t[0], ctrl) and np.array_equal(t[2], kcount)


def test_affine_landmark_maps_give_the_affine_rows_and_no_bending():
    rng = np.random.RandomState(2)
    src = distinct_points(rng, 20, 48, 48)[None]
    th, sc, shift = 0.3, 1.1, np.array([2.5, -1.25])
    A = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    ref = src @ A.T + shift
    ctrl, coef, kcount = teacher.tps_coefficients(src, ref)
    assert kcount.tolist() == [20] and coef.shape == (1, 2, 23)
    assert np.abs(coef[0, :, :20]).max() <= 1e-9
    assert np.abs(coef[0, :, 20] - shift).max() <= 1e-8 and np.abs(coef[0, :, 21:] - A).max() <= 1e-9


def test_duplicates_are_dropped_and_degenerate_samples_keep_the_hist_image():
    rng = np.random.RandomState(3)
    base = distinct_points(rng, 10, 32, 32)
    src = np.concatenate([base[:4], base[1:2], base[4:], base[:1]])[None]          # points 1 and 0 repeated
    ref = src + rng.uniform(-2, 2, src.shape)
    ctrl, coef, kcount = teacher.tps_coefficients(src, ref)
    assert kcount.tolist() == [10] and np.array_equal(ctrl[0, :10], base) and ctrl.shape == (1, 12, 2)
    want = teacher.tps_coefficients(base[None], np.concatenate([ref[0, :4], ref[0, 5:11]])[None], max_ctrl=12)          # the first of each is kept
    assert np.array_equal(coef, want[1])
    line = np.stack([np.arange(6.0), 2 * np.arange(6.0)], 1)[None]
    nan = base[None].copy()
    nan[0, 3, 1] = np.nan
    inf = base[None].copy()
    inf[0, 0, 0] = np.inf
    two = np.concatenate([base[:2]] * 3)[None]                                      # two distinct points
    for s, r in ((line, line + 1.0), (nan, base[None]), (base[None], nan), (base[None], inf), (two, two), (base[None, :2], base[None, :2])):
        c, f, k = teacher.tps_coefficients(s, r)
        assert k.tolist() == [0] and not c.any() and not f.any()
    # one bad sample does not spoil its neighbours
    c, f, k = teacher.tps_coefficients(np.concatenate([nan, base[None]]), np.concatenate([base[None], base[None] + 1.0]))
    assert k.tolist() == [0, 10] and np.abs(f[1, :, 10] - 1.0).max() <= 1e-8
    for bad in ((base, base), (base[None], base[None, :5]), (base[None, :, :1], base[None, :, :1])):
        with pytest.raises(ValueError):
            teacher.tps_coefficients(*bad)
    with pytest.raises(ValueError):
        teacher.tps_coefficients(base[None], base[None], max_ctrl=9)
    with pytest.raises(ValueError):
        teacher.tps_coefficients(base[None], base[None], max_ctrl=129)


# ---- 2. the definition, where the answer is known ------------------------------------------------------------------------------------
def full_masks(n, H, W):
    m = np.zeros((4, n, H, W), dtype=np.uint8)
    m[0] = 1          # everything is lip
    return m


@pytest.mark.parametrize('shift', [0, 1, -3, 5])
def test_a_horizontal_ramp_under_an_integer_shift(shift):
    H, W = 9, 14
    ramp = np.broadcast_to((np.arange(W) / 64).astype(np.float32), (1, 3, H, W)).copy()
    xh = np.full((1, 3, H, W), 0.8125, np.float32)
    ctrl, coef, kcount = wr.affine_spline(1, 4, ((0, 1, 0), (shift, 0, 1)))
    ones = np.ones((1, 4), np.float32)
    out, q = wr.warp(xh, ramp, full_masks(1, H, W), full_masks(1, H, W), ctrl, coef, kcount, ones, 0, want_map=True)
    assert np.array_equal(q[0, 0], np.mgrid[0:H, 0:W][0]) and np.array_equal(q[0, 1], np.mgrid[0:H, 0:W][1] + shift)
    xs = np.arange(W) + shift
    inside = (xs >= 0) & (xs <= W - 1)
    assert np.array_equal(out[0, :, :, inside], np.broadcast_to((xs[inside] / 64).astype(np.float32)[:, None, None], (inside.sum(), 3, H)))
    assert np.array_equal(out[0, :, :, ~inside].view(np.uint32), xh[0, :, :, ~inside].view(np.uint32))          # q_x = -1 or W and beyond: xh
    # alpha scales the step towards the reference; alpha 0 and K = 0 return xh bit for bit
    half = wr.warp(xh, ramp, full_masks(1, H, W), full_masks(1, H, W), ctrl, coef, kcount, ones * 0.5, 0)
    assert np.array_equal(half[0, :, :, inside], (0.8125 + 0.5 * (out[0, :, :, inside].astype(np.float64) - 0.8125)).astype(np.float32))
    for kw in (dict(alphas=ones * 0), dict(kcount=np.zeros(1, np.int32))):
        args = dict(ctrl=ctrl, coef=coef, kcount=kcount, alphas=ones)
        args.update(kw)
        same = wr.warp(xh, ramp, full_masks(1, H, W), full_masks(1, H, W), feather=0, **args)
        assert np.array_equal(same.view(np.uint32), xh.view(np.uint32))


def test_a_ramp_under_an_affine_map():
    """bilinear sampling of a plane (x + 2 y) / 256 at q = (0.5 y + 1, 0.25 x + 2.5) is the plane at q: every operand is a dyadic rational"""
    H, W = 12, 20
    yy, xx = np.mgrid[0:H, 0:W]
    ref = np.broadcast_to(((xx + 2 * yy) / 256).astype(np.float32), (1, 3, H, W)).copy()
    xh = np.zeros((1, 3, H, W), np.float32)
    ctrl, coef, kcount = wr.affine_spline(1, 3, ((1, 0.5, 0), (2.5, 0, 0.25)))
    out, q = wr.warp(xh, ref, full_masks(1, H, W), full_masks(1, H, W), ctrl, coef, kcount, np.ones((1, 4), np.float32), 0, want_map=True)
    assert np.array_equal(q[0, 0], 0.5 * yy + 1) and np.array_equal(q[0, 1], 0.25 * xx + 2.5)
    assert q[0, 0].max() <= H - 1 and q[0, 1].max() <= W - 1                         # every tap is inside: Wt = 1 everywhere
    assert np.array_equal(out[0], np.broadcast_to(((q[0, 1] + 2 * q[0, 0]) / 256).astype(np.float32), (3, H, W)))
    # a source region of one pixel with feather 1 spreads the weight c / 9 over its 3 x 3 neighbourhood
    m = np.zeros((4, 1, H, W), dtype=np.uint8)
    m[1, 0, 5, 7] = 1
    soft = wr.warp(xh, ref, m, full_masks(1, H, W) * 0 + 1, ctrl, coef, kcount, np.ones((1, 4), np.float32), 1)
    want = np.zeros((H, W))
    want[4:7, 6:9] = 1.0 / 9.0
    assert np.array_equal(soft[0, 0], (want * out[0, 0].astype(np.float64)).astype(np.float32))


def test_reference_validity_follows_the_reference_masks_and_nan_is_no_position():
    H, W = 8, 8
    ref = np.full((1, 3, H, W), 1.0, np.float32)
    ref[0, 0, 0, 0] = np.nan                                                         # NaN colour counts as 0
    xh = np.zeros((1, 3, H, W), np.float32)
    rm = np.zeros((4, 1, H, W), dtype=np.uint8)
    rm[0, 0, :, 4:] = 1                                                              # the reference has lips on its right half only
    ctrl, coef, kcount = wr.affine_spline(1, 3, ((0, 1, 0), (0.5, 0, 1)))            # half a pixel to the right
    out = wr.warp(xh, ref, full_masks(1, H, W), rm, ctrl, coef, kcount, np.ones((1, 4), np.float32), 0)
    assert not out[0, :, :, :3].any() and np.all(out[0, 1, :, 3] == 0.5) and np.all(out[0, :, :, 4:7] == 1.0)
    assert np.all(out[0, 1, :, 7] == 0.5)                                            # the right tap is outside the image: 0
    coef[0, 0, 3] = np.nan
    assert not wr.warp(xh, ref, full_masks(1, H, W), rm, ctrl, coef, kcount, np.ones((1, 4), np.float32), 0).any()
    coef[0, 0, 3] = 1e300
    assert not wr.warp(xh, ref, full_masks(1, H, W), rm, ctrl, coef, kcount, np.ones((1, 4), np.float32), 0).any()


# ---- 3. the C entry ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_bad_arguments_without_a_device():
    lib = mlib.load()
    buf = (C.c_float * 8192)()
    xh, ref, out = C.addressof(buf), C.addressof(buf) + 4 * 2048, C.addressof(buf) + 4 * 4096
    mbuf = (C.c_uint8 * 4096)()
    m = C.addressof(mbuf)
    dbuf = (C.c_double * 2048)()
    d = C.addressof(dbuf)
    ptrs = ('xh', 'ref', 'src_masks', 'ref_masks', 'ctrl', 'coef', 'kcount', 'alphas', 'out', 'map_out')
    ok = dict(xh=xh, ref=ref, src_masks=m, ref_masks=m, ctrl=d, coef=d + 8 * 512, kcount=d + 8 * 1024, alphas=d + 8 * 1100, n=1, H=8, W=8, max_ctrl=68,
              feather=2, out=out, map_out=None)
    call = lambda **kw: lib.mkd_pgt_warp(*[C.c_void_p(v) if k in ptrs else v for k, v in {**ok, **kw}.items()], None)
    bad = [{k: None} for k in ptrs[:-1]]
    bad += [dict(n=0), dict(n=65536), dict(H=0), dict(W=0), dict(W=-8), dict(H=4097, W=4096), dict(feather=-1), dict(feather=9), dict(max_ctrl=0),
            dict(max_ctrl=129), dict(xh=xh + 2), dict(ref=ref + 1), dict(out=out + 2), dict(alphas=d + 2), dict(kcount=d + 1), dict(ctrl=d + 4), dict(coef=d + 4),
            dict(map_out=d + 4),
            dict(out=ref), dict(out=ref + 4 * 100), dict(out=ref - 4 * 100),          # out overlaps ref
            dict(out=xh + 4 * 100), dict(xh=out + 4 * 191), dict(out=xh + 4 * 191)]   # out overlaps xh without being xh
    for kw in bad:
        assert call(**kw) == -1 and lib.mkd_last_error(), kw          # MKD_ERR_ARG
    assert lib.mkd_pgt_warp_launches() == 1
    assert teacher.launches() == 16 and teacher.launches(warp=False) == 16 and teacher.launches(warp=True) == 17


# ---- 4. host rules -----------------------------------------------------------------------------------------------------------------------
def test_alpha_rows_forms_and_refusals():
    assert teacher.alpha_rows(None, 2) is None and teacher.alpha_rows(False, 2) is None
    assert teacher.REFERENCE_ALPHAS == dict(skin=0.3, eye=0.8, lip=0.1)
    ref = torch.tensor([[0.1, 0.3, 0.8, 0.8]] * 2)                                  # lip, skin, eye_left, eye_right
    assert torch.equal(teacher.alpha_rows(True, 2), ref) and torch.equal(teacher.alpha_rows({}, 2), ref)
    r = teacher.alpha_rows({'eye': [0.0, 1.0], 'lip': 0.5}, 2)
    assert r.dtype == torch.float32 and torch.equal(r, torch.tensor([[0.5, 0.3, 0.0, 0.0], [0.5, 0.3, 1.0, 1.0]]))
    for bad in ({'lip': 1.5}, {'skin': -0.1}, {'eye': float('nan')}, {'nose': 0.5}, {'lip': [0.1, 0.2, 0.3]}, 0.5, 'on', [0.1, 0.8, 0.3]):
        with pytest.raises(ValueError):
            teacher.alpha_rows(bad, 2)


def test_warp_needs_both_landmark_arrays():
    x = torch.zeros(1, 3, 8, 8)
    seg = torch.zeros(1, 8, 8, dtype=torch.uint8)
    lms = torch.tensor([[[1.0, 1.0], [5.0, 2.0], [3.0, 6.0]]])
    for kw in (dict(), dict(lms_src=lms), dict(lms_ref=lms)):
        with pytest.raises(ValueError, match='landmarks'):
            teacher.pseudo_ground_truth(x, x, seg, seg, warp=True, **kw)
    with pytest.raises(ValueError):
        teacher.pseudo_ground_truth(x, x, seg, seg, warp={'lip': 2.0}, lms_src=lms, lms_ref=lms)
    with pytest.raises(ValueError):
        teacher.pseudo_ground_truth(x, x, seg, seg, warp=True, lms_src=lms.repeat(2, 1, 1), lms_ref=lms.repeat(2, 1, 1))
    with pytest.raises(mlib.MkdError):          # off: the call is the old one, and there is no CPU path
        teacher.pseudo_ground_truth(x, x, seg, seg, warp=False, lms_src=lms, lms_ref=lms)
    with pytest.raises(mlib.MkdError):
        teacher.warp_blend(x, x, torch.zeros(4, 1, 8, 8, dtype=torch.uint8), torch.zeros(4, 1, 8, 8, dtype=torch.uint8), torch.zeros(1, 3, 2, dtype=torch.float64),
                           torch.zeros(1, 2, 6, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4))


# ---- 5. the model, the dataset and the command line ---------------------------------------------------------------------------------
def _model(**attrs):
    from makeupdiffuse_amd.config import create_model
    m = create_model(os.path.join(ROOT, 'diffmodels', 'test_diffusion_makeup.yaml'))

    def no_engine():
        raise AssertionError('the engine was reached: the refusal came too late')
    m._require_engine = no_engine
    m.save_images = False
    m.ddim_steps = 10
    for k, v in {'teacher': 'hist', **attrs}.items():
        setattr(m, k, v)
    return m


def _batch(m, B=2):
    g = torch.Generator().manual_seed(5)
    lms = torch.tensor([[2.0, 2.0], [12.0, 3.0], [4.0, 13.0], [11.0, 11.0]]).expand(B, -1, -1).contiguous()
    return {'src_img': torch.rand(B, 3, 16, 16, generator=g), 'ref_img': torch.rand(B, 3, 16, 16, generator=g),
            'txt_emb': torch.randn(B, 77, m.net_config.context_dim, generator=g), m.seg_key: torch.ones(B, 16, 16, dtype=torch.uint8),
            m.ref_seg_key: torch.ones(B, 16, 16, dtype=torch.uint8), m.lms_key: lms, m.ref_lms_key: lms + 1.0}


def test_model_keyword_checks_and_refusals():
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    for bad in (dict(teacher_warp=True), dict(teacher_warp={'eye': 0.5}), dict(teacher='hist', teacher_warp={'eye': 1.5}),
                dict(teacher='hist', teacher_warp={'brow': 0.5}), dict(teacher='hist', teacher_warp=0.5)):
        with pytest.raises(ValueError):
            TestDiffuseModel(**bad)                          # (checked before anything is built)
    m = _model(teacher_warp=True)
    assert (m.lms_key, m.ref_lms_key) == ('nonmakeup_lms', 'makeup_lms')
    for drop in (m.lms_key, m.ref_lms_key):
        b = _batch(m)
        del b[drop]
        with pytest.raises(ValueError, match=f"landmarks of the source and of the reference.*'{drop}'"):
            m.log_results(b, 0)
    photo = [torch.zeros(32, 32, 3, dtype=torch.uint8)]
    box = [(0, 0, 32, 32)]
    seg = [torch.zeros(32, 32, dtype=torch.uint8)]
    with pytest.raises(ValueError, match='teacher_start is not combined with teacher_warp'):
        m.transfer_photos(photo, photo, box, box, src_segs=seg, ref_segs=seg, teacher_start=0.5)


def test_dataset_brings_landmarks_at_the_model_size(tmp_path):
    from PIL import Image
    from makeupdiffuse_amd.imageio import PairFolderDataset, collate
    os.makedirs(tmp_path / 'images')
    for name in ('a.png', 'b.png'):
        Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(tmp_path / 'images' / name)
    (tmp_path / 'pairs.txt').write_text('a.png b.png\n')
    assert 'nonmakeup_lms' not in PairFolderDataset(str(tmp_path), 'pairs.txt', (32, 32))[0]
    os.makedirs(tmp_path / 'lms')
    la, lb = np.array([[1, 2], [30, 4], [5, 31]], dtype=np.int32), np.array([[10, 20], [60, 8], [10, 62]], dtype=np.int32)
    np.save(tmp_path / 'lms' / 'a.npy', la)
    np.save(tmp_path / 'lms' / 'b.npy', lb)
    (tmp_path / 'lms' / 'sizes.json').write_text(json.dumps({'b': 64}))          # b's landmarks were stored for the 64 x 64 image
    ds = PairFolderDataset(str(tmp_path), 'pairs.txt', (32, 32))
    item = ds[0]
    assert ds.has_lms and item['nonmakeup_lms'].dtype == torch.float32
    assert torch.equal(item['nonmakeup_lms'], torch.from_numpy(la).float())      # no size entry: taken as given at the model size
    assert torch.equal(item['makeup_lms'], torch.from_numpy(lb).float() / 2)
    assert tuple(collate([item, item])['makeup_lms'].shape) == (2, 3, 2)


def test_cli_accepts_the_warp_flags_only_with_the_hist_teacher_and_the_pair_passes():
    cli = [sys.executable, os.path.join(ROOT, 'runs', 'test.py')]
    for more, word in ((['--teacher-warp'], 'only apply with --teacher hist'),
                       (['--teacher', 'hist', '--teacher-warp-alphas', '0.1,0.8,0.3'], '--teacher-warp-alphas only applies with --teacher-warp'),
                       (['--teacher', 'hist', '--teacher-warp', '--teacher-warp-alphas', '0.1,0.8'], 'three numbers'),
                       (['--teacher', 'hist', '--teacher-warp', '--teacher-warp-alphas', '0.1,1.8,0.3'], 'three numbers'),
                       (['--teacher', 'hist', '--teacher-warp', '--video', 'clip', '--video-ref', 'ref.png'], '--teacher-warp is not combined with --video')):
        r = subprocess.run(cli + more, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and word in r.stderr, (more, r.stderr[-400:])
    import importlib.util
    spec = importlib.util.spec_from_file_location('mkd_runs_test', os.path.join(ROOT, 'runs', 'test.py'))
    cli_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli_mod)
    lms = cli_mod.synthetic_lms(3, 64)
    seg = cli_mod.synthetic_seg(3, 64, True)
    assert lms.dtype == torch.float32 and lms.shape[1] == 2 and lms.shape[0] >= 12 and len({tuple(p) for p in lms.tolist()}) == lms.shape[0]
    centre = lambda lab: torch.nonzero(seg == lab).float().mean(0)
    assert (lms[5] - centre(4)).abs().max() <= 1.0 and (lms[10] - centre(5)).abs().max() <= 1.0          # the eye blobs' centres
    assert teacher.tps_coefficients(lms[None], cli_mod.synthetic_lms(7003, 64)[None])[2].tolist() == [lms.shape[0]]
    b = cli_mod.synthetic_batch(0, 2, 32, 8, with_makeup_seg=True, with_lms=True)
    assert tuple(b['nonmakeup_lms'].shape) == tuple(b['makeup_lms'].shape) == (2, lms.shape[0], 2)
    assert 'nonmakeup_lms' not in cli_mod.synthetic_batch(0, 2, 32, 8, with_makeup_seg=True)
