"""CPU: control points from region masks and the spline solve of the warped teacher.  The restatement (tests/teacher_points_ref.py, what
mkd_region_points and mkd_tps_solve are held to on the device) against the host solve teacher.tps_coefficients on synthetic faces, the
refusals of the two C entries, of the keywords and of the command line that need no device, the launch counts and the ABI version."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import teacher_points_ref as pr
import teacher_warp_ref as wr
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import teacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_solve(ps, pf, us, uf, M):
    """teacher.tps_coefficients of ONE sample's pairs in use"""
    on = (us != 0) & (uf != 0)
    c, f, k = teacher.tps_coefficients(ps[on][None], pf[on][None], max_ctrl=M) if on.any() else (np.zeros((1, M, 2)), np.zeros((1, 2, M + 3)), [0])
    return c[0], f[0], int(k[0])


# ---- 1. the points ---------------------------------------------------------------------------------------------------------------------
def test_region_points_on_cases_with_a_known_answer():
    m = np.zeros((4, 1, 6, 9), dtype=np.uint8)
    m[0, 0, 1:4, 2:7] = 200          # lip: a rectangle, whole edges tie
    m[1, 0] = 1                      # skin everywhere: what is left of it after the lip and the eye
    m[2, 0, 5, 8] = 1                # eye_left: one pixel in the corner
    pts, use, count = pr.region_points_ref(m, 8, 1)
    assert pts.shape == (1, 36, 2) and use.shape == (1, 36) and count.tolist() == [[15, 1, 0, 54 - 16]]
    assert use[0].tolist() == [1] * 18 + [0] * 9 + [1] * 9
    assert pts[0, 0].tolist() == [2.0, 4.0]
    # d = 0 (+x): the right edge ties, its top pixel has the smallest index; d = 2 (+y): the bottom edge, its left pixel; d = 4 (-x), d = 6 (-y)
    assert pts[0, 1].tolist() == [1.0, 6.0] and pts[0, 3].tolist() == [3.0, 2.0] and pts[0, 5].tolist() == [1.0, 2.0] and pts[0, 7].tolist() == [1.0, 2.0]
    assert pts[0, 2].tolist() == [3.0, 6.0] and pts[0, 4].tolist() == [3.0, 2.0]          # the diagonals take the corners
    assert (pts[0, 9:18] == [5.0, 8.0]).all() and not pts[0, 18:27].any()                  # one pixel: every point is it; empty: zeros
    big = pr.region_points_ref(m, 8, 16)
    assert big[1][0].tolist() == [0] * 27 + [1] * 9 and not big[0][0, :27].any() and np.array_equal(big[2], count)
    p16 = pr.region_points_ref(m, 16, 1)[0]
    assert np.array_equal(p16[0, 1:17:2], pts[0, 1:9]) and p16.shape == (1, 68, 2)          # D = 8 is every second direction of 16
    assert [tuple(d) for d in pr.directions(16)[5:9]] == [(-c, s) for c, s in pr.directions(16)[3::-1]]
    assert [tuple(d) for d in pr.directions(16)[9:]] == [(-c, -s) for c, s in pr.directions(16)[1:8]]


@pytest.mark.parametrize('shape', [(64, 64), (40, 24)])
@pytest.mark.parametrize('dirs', [8, 16])
def test_mask_points_of_synthetic_pairs_give_a_spline_the_host_accepts(shape, dirs):
    H, W = shape
    ps, pf, us, uf = pr.paired_points(pr.face_pairs(H, W), dirs)
    K = 4 * (dirs + 1)
    assert ps.shape == (20, K, 2) and us.all() and uf.all()          # every region of every face has min_area pixels
    distinct = []
    for b in range(len(ps)):
        c, f, k = host_solve(ps[b], pf[b], us[b], uf[b], K)
        assert k >= 3, (b, k)
        distinct.append(k)
        q = wr.spline_map(c[None], f[None], [k], H, W)[0]
        at = c[:k].astype(int)          # support points are pixels; centroids are not: only the former are looked up
        whole = (c[:k] == at).all(1)
        want = pf[b][[int(np.nonzero((ps[b] == p).all(1))[0][0]) for p in c[:k]]]
        assert np.abs(q[:, at[whole, 0], at[whole, 1]].T - want[whole]).max() <= 1e-6
    print(f'{H} x {W}, D = {dirs}: {K} pairs, {min(distinct)} .. {max(distinct)} distinct control points')


def test_a_region_below_min_area_on_one_side_drops_its_pairs_on_both():
    m = pr.face_pairs(64, 64)[:, [0, 20]]          # one pair: [src | ref]
    ref_eye = m[2, 1].copy()
    y, x = np.nonzero(ref_eye)
    m[2, 1] = 0
    m[2, 1, y[:3], x[:3]] = 1                       # the reference's left eye keeps three pixels
    ps, pf, us, uf = pr.paired_points(m, 16, 4)
    assert us.all() and uf[0].tolist() == [1] * 17 + [0] * 17 + [1] * 34
    c, d = pr.kept_pairs(ps[0], pf[0], us[0], uf[0])
    rest = np.r_[0:17, 34:68]
    c2, d2 = pr.kept_pairs(ps[0][rest], pf[0][rest])
    assert np.array_equal(c, c2) and np.array_equal(d, d2)
    eye = {tuple(p) for p in ps[0, 17:34]}
    assert not eye & {tuple(p) for p in c}
    got, want = pr.solve_ref(ps, pf, us, uf), teacher.tps_coefficients(ps[:, rest], pf[:, rest], max_ctrl=68)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and got[2][0] >= 3
    assert pr.paired_points(m, 16, 3)[3].all()      # three pixels are enough for min_area = 3


# ---- 2. the solve ----------------------------------------------------------------------------------------------------------------------
def test_the_restated_solve_and_the_host_solve_agree():
    for name, H, W, src, ref in pr.solve_cases():
        K = src.shape[1]
        for M in (K, 128):
            a, b = pr.solve_ref(src, ref, max_ctrl=M), teacher.tps_coefficients(src, ref, max_ctrl=M)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[2].tolist() == [K, K], name
            assert np.allclose(a[1], b[1], rtol=0, atol=1e-9 * max(1.0, np.abs(b[1]).max())), name
            for s in range(2):
                assert pr.full_residual(a[0][s], a[1][s], K, ref[s]) <= pr.TPS_RESIDUAL
                assert pr.full_residual(b[0][s], b[1][s], K, ref[s]) <= pr.TPS_RESIDUAL          # the host's passes the full-system test too
    for H, W in ((64, 64), (40, 24)):
        ps, pf, us, uf = pr.paired_points(pr.face_pairs(H, W))
        got = pr.solve_ref(ps, pf, us, uf)
        for b in range(len(ps)):
            c, f, k = host_solve(ps[b], pf[b], us[b], uf[b], 68)
            assert np.array_equal(got[0][b], c) and got[2][b] == k >= 3
    d = pr.delta_ref()
    print(f'Delta_ref = {d:.3e} px (the maps of the restated and of the host solve over solve_cases)')
    assert 0.0 < d < pr.TPS_RESIDUAL


def test_degenerate_samples_are_dropped_by_both():
    rng = np.random.RandomState(3)
    flat = rng.choice(32 * 32, 10, replace=False)
    base = np.stack([flat // 32, flat % 32], 1).astype(np.float64)
    line = np.stack([np.arange(2.0, 14.0, 2.0), np.zeros(6)], 1)          # x = 0: collinear
    nan = base.copy()
    nan[3, 1] = np.nan
    inf = base.copy()
    inf[0, 0] = np.inf
    two = np.concatenate([base[:2]] * 3)
    for s, r in ((line, line + 1.0), (nan, base), (base, nan), (base, inf), (two, two), (base[:2], base[:2])):
        for fn in (pr.solve_ref, teacher.tps_coefficients):
            c, f, k = fn(s[None], r[None])
            assert k.tolist() == [0] and not c.any() and not f.any(), fn
    # repeated points: the first is kept, as on the host; a NaN in a pair that is not in use does not count
    rep = np.concatenate([base[:4], base[1:2], base[4:], base[:1]])
    ref = rep + rng.uniform(-2, 2, rep.shape)
    a, b = pr.solve_ref(rep[None], ref[None]), teacher.tps_coefficients(rep[None], ref[None])
    assert a[2].tolist() == b[2].tolist() == [10] and np.array_equal(a[0], b[0]) and np.array_equal(a[0][0, :10], base)
    use = np.ones((1, 10), np.int32)
    use[0, 3] = 0
    a = pr.solve_ref(nan[None], base[None] + 1.0, use, None)
    assert a[2].tolist() == [9] and np.isfinite(a[1]).all()
    assert pr.solve_ref(nan[None], base[None] + 1.0, None, use)[2].tolist() == [9]
    # a bad sample between two good ones
    c, f, k = pr.solve_ref(np.stack([base, line[[0, 1, 2, 3, 4, 5, 0, 1, 2, 3]], base]), np.stack([base + 1.0, base, base - 1.0]))
    assert k.tolist() == [10, 0, 10] and not c[1].any() and not f[1].any()
    assert np.abs(f[0, :, 10] - 1.0).max() <= 1e-8 and np.abs(f[2, :, 10] + 1.0).max() <= 1e-8


# ---- 3. the C entries ------------------------------------------------------------------------------------------------------------------
def test_region_points_refuses_bad_arguments_without_a_device():
    lib = mlib.load()
    buf = (C.c_uint8 * (1 << 16))()
    base = (C.addressof(buf) + 255) & ~255
    ptrs = ('masks', 'pts', 'use', 'count', 'scratch')
    ok = dict(masks=base, n=1, H=8, W=8, dirs=16, min_area=4, pts=base + 4096, use=base + 8192, count=base + 12288, scratch=base + 16384)
    call = lambda **kw: lib.mkd_region_points(*[C.c_void_p(v) if k in ptrs else v for k, v in {**ok, **kw}.items()], None)
    bad = [{k: None} for k in ptrs if k != 'count']
    bad += [dict(n=0), dict(n=65536), dict(n=-1), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(H=-8), dict(dirs=0), dict(dirs=4), dict(dirs=12),
            dict(dirs=32), dict(min_area=0), dict(min_area=-3), dict(scratch=base + 16384 + 128), dict(scratch=base + 16384 + 8), dict(pts=base + 4100),
            dict(use=base + 8194), dict(count=base + 12289)]
    for kw in bad:
        assert call(**kw) == -1 and lib.mkd_last_error(), kw          # MKD_ERR_ARG, before any launch: there is no device here
    assert lib.mkd_region_points_launches() == 3
    assert lib.mkd_region_points_scratch_bytes(0) == 0 and lib.mkd_region_points_scratch_bytes(65536) == 0
    for n in (1, 2, 3, 65535):
        b = lib.mkd_region_points_scratch_bytes(n)
        assert b % 256 == 0 and n * 4 * 19 * 8 <= b < n * 4 * 19 * 8 + 256


def test_tps_solve_refuses_bad_arguments_without_a_device():
    lib = mlib.load()
    dbuf = (C.c_double * 8192)()
    d = C.addressof(dbuf)
    ptrs = ('pts_src', 'pts_ref', 'use_src', 'use_ref', 'ctrl', 'coef', 'kcount')
    ok = dict(pts_src=d, pts_ref=d + 8 * 1024, use_src=None, use_ref=None, B=1, K=68, max_ctrl=68, ctrl=d + 8 * 2048, coef=d + 8 * 3072, kcount=d + 8 * 4096)
    call = lambda **kw: lib.mkd_tps_solve(*[C.c_void_p(v) if k in ptrs else v for k, v in {**ok, **kw}.items()], None)
    bad = [{k: None} for k in ptrs if not k.startswith('use')]
    bad += [dict(B=0), dict(B=65536), dict(B=-2), dict(K=0), dict(K=-1), dict(K=69), dict(K=129, max_ctrl=129), dict(max_ctrl=129), dict(max_ctrl=67),
            dict(K=1, max_ctrl=0), dict(pts_src=d + 4), dict(pts_ref=d + 8 * 1024 + 4), dict(ctrl=d + 8 * 2048 + 4), dict(coef=d + 8 * 3072 + 1),
            dict(kcount=d + 8 * 4096 + 4), dict(use_src=d + 8 * 5000 + 2), dict(use_ref=d + 8 * 5000 + 1)]
    for kw in bad:
        assert call(**kw) == -1 and lib.mkd_last_error(), kw
    assert lib.mkd_tps_solve_launches() == 1


def test_launch_counts_and_the_abi_version():
    assert mlib.ABI_VERSION == 1 and mlib.load().mkd_abi_version() == 1
    assert teacher.launches() == 16 and teacher.launches(warp=False) == 16 and teacher.launches(warp=True) == 17          # the two existing forms
    assert teacher.launches(warp=True, points=None, solve='host') == 17
    assert teacher.launches(warp=True, solve='device') == 18 and teacher.launches(warp=True, points='masks') == 21
    assert teacher.launches(warp=True, points='masks', solve='device') == 21
    assert teacher.launches(warp=False, points='masks') == 16
    for bad in (dict(points='lms'), dict(solve='gpu')):
        with pytest.raises(ValueError):
            teacher.launches(warp=True, **bad)


# ---- 4. the keywords -------------------------------------------------------------------------------------------------------------------
def test_keyword_checks_come_before_the_device():
    x = torch.zeros(1, 3, 8, 8)
    seg = torch.zeros(1, 8, 8, dtype=torch.uint8)
    lms = torch.tensor([[[1.0, 1.0], [5.0, 2.0], [3.0, 6.0]]])
    for kw in (dict(warp=True, points='lms'), dict(warp=True, points='masks', point_dirs=12), dict(warp=True, solve='gpu', lms_src=lms, lms_ref=lms),
               dict(points='masks'), dict(warp=False, solve='device'), dict(warp=True, points='masks', lms_src=lms, lms_ref=lms),
               dict(warp=True, points='masks', point_dirs=True), dict(warp=True, solve='device'), dict(warp=True, solve='device', lms_src=lms),
               dict(warp=True, solve='device', lms_src=lms, lms_ref=lms[:, :2]), dict(warp=True, solve='device', lms_src=lms.repeat(2, 1, 1), lms_ref=lms.repeat(2, 1, 1))):
        with pytest.raises(ValueError):
            teacher.pseudo_ground_truth(x, x, seg, seg, **kw)
    for kw in (dict(warp=True, points='masks'), dict(warp=True, solve='device', lms_src=lms, lms_ref=lms)):
        with pytest.raises(mlib.MkdError):          # the keywords are fine: there is no CPU path
            teacher.pseudo_ground_truth(x, x, seg, seg, **kw)
    with pytest.raises(mlib.MkdError):
        teacher.region_points(torch.zeros(4, 1, 8, 8, dtype=torch.uint8))
    with pytest.raises(mlib.MkdError):
        teacher.tps_coefficients_device(lms, lms)


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


def test_model_keyword_checks_and_refusals():
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    for bad in (dict(teacher='hist', teacher_points='masks'), dict(teacher='hist', teacher_warp=False, teacher_points='masks'),
                dict(teacher='hist', teacher_warp=True, teacher_points='lms'), dict(teacher='hist', teacher_warp=True, teacher_points='masks', teacher_point_dirs=4),
                dict(teacher='hist', teacher_warp=True, teacher_point_dirs=8), dict(teacher_warp=True, teacher_points='masks')):
        with pytest.raises(ValueError):
            TestDiffuseModel(**bad)                          # (checked before anything is built)
    m = _model(teacher_warp=True)
    assert m.teacher_points is None and m.teacher_point_dirs == 16 and m._mask_points_warp() == {}
    photo = [torch.zeros(32, 32, 3, dtype=torch.uint8)]
    box = [(0, 0, 32, 32)]
    seg = [torch.zeros(32, 32, dtype=torch.uint8)]
    with pytest.raises(ValueError, match='teacher_start is not combined with teacher_warp'):          # without 'masks': the present refusal
        m.transfer_photos(photo, photo, box, box, src_segs=seg, ref_segs=seg, teacher_start=0.5)
    m.teacher_points, m.teacher_point_dirs = 'masks', 8
    assert m._mask_points_warp() == dict(warp=True, points='masks', point_dirs=8)
    with pytest.raises(Exception) as e:                      # with it the call goes on to what it needs next (here: an encoder)
        m.transfer_photos(photo, photo, box, box, src_segs=seg, ref_segs=seg, teacher_start=0.5)
    assert 'teacher_warp' not in str(e.value)
    batch = {'src_img': torch.rand(2, 3, 16, 16), 'ref_img': torch.rand(2, 3, 16, 16), 'txt_emb': torch.randn(2, 77, m.net_config.context_dim),
             m.seg_key: torch.ones(2, 16, 16, dtype=torch.uint8), m.ref_seg_key: torch.ones(2, 16, 16, dtype=torch.uint8)}
    m._check_teacher(batch, None)                            # no landmark keys are asked for
    m.teacher_points = None
    with pytest.raises(ValueError, match='landmarks of the source and of the reference'):
        m._check_teacher(batch, None)


def test_cli_flags():
    cli = [sys.executable, os.path.join(ROOT, 'runs', 'test.py')]
    hist = ['--teacher', 'hist']
    for more, word in ((hist + ['--teacher-points', 'masks'], '--teacher-points only applies with --teacher-warp'),
                       (hist + ['--teacher-warp', '--teacher-point-dirs', '8'], '--teacher-point-dirs only applies with --teacher-points masks'),
                       (hist + ['--teacher-warp', '--teacher-points', 'masks', '--teacher-point-dirs', '12'], 'invalid choice'),
                       (hist + ['--teacher-warp', '--teacher-points', 'lms'], 'invalid choice'),
                       (['--teacher-warp', '--teacher-points', 'masks'], 'only apply with --teacher hist'),
                       (hist + ['--teacher-warp', '--photos', '--data-root', 'nowhere'], '--teacher-warp is not combined with --photos'),
                       (hist + ['--teacher-warp', '--teacher-points', 'masks', '--video', 'clip', '--video-ref', 'ref.png'],
                        '--teacher-warp is not combined with --video'),
                       (hist + ['--teacher-warp', '--teacher-points', 'masks', '--region-refs', 'lip=a.png', '--data-root', 'nowhere', '--face-parser', 'random'],
                        '--teacher-warp is not combined with --region-refs')):
        r = subprocess.run(cli + more, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and word in r.stderr, (more, r.stderr[-400:])
    # with the mask points --photos passes the teacher checks: the run stops at the first thing it needs after them (the data root)
    r = subprocess.run(cli + hist + ['--teacher-warp', '--teacher-points', 'masks', '--photos', '--data-root', 'nowhere'], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '--teacher-warp is not combined' not in r.stderr, r.stderr[-400:]
