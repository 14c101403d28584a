"""-m gpu: control points from region masks and the spline solve on the device.  (a) mkd_region_points against the restatement
(tests/teacher_points_ref.py) byte for byte over pts, use and count; (b) mkd_tps_solve: ctrl and kcount bit for bit against
teacher.tps_coefficients, the full-system residual of the device's coefficients, its map against the host's within 16 Delta_ref, the
degenerate samples, the same bytes twice; (c) teacher.pseudo_ground_truth(points=, solve=) against the chain of its pieces."""
import numpy as np
import pytest
import torch

import teacher_points_ref as pr
import teacher_ref as tr
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import makeup_score as ms
from makeupdiffuse_amd import teacher

pytestmark = pytest.mark.gpu

PAD = 64          # canary elements on both sides of the outputs
# the issue's sizes, plus two with an odd W: 33 x 37 = 1221 pixels is two workgroups (1024 pixels each) whose border cuts a row
SHAPES = [(8, 8), (24, 40), (40, 24), (64, 64), (17, 33), (33, 37)]


def canaried(count, dtype, fill):
    buf = torch.full((PAD + count + PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + count]


def inside(buf, count, fill, what):
    got = buf.cpu().numpy()
    assert (got[:PAD] == fill).all() and (got[PAD + count:] == fill).all(), f'wrote outside {what}'
    return got[PAD:PAD + count]


def run_points(masks, dirs, min_area, off=0, want_count=True):
    """mkd_region_points with the masks `off` bytes past a 256-byte aligned base, the outputs between canaries -> numpy"""
    _, n, H, W = masks.shape
    K = 4 * (dirs + 1)
    mbuf = torch.zeros(masks.size + off + 64, dtype=torch.uint8, device=DEV)
    m = mbuf[off:off + masks.size]
    m.copy_(torch.from_numpy(np.ascontiguousarray(masks).reshape(-1)))
    pb, p = canaried(n * K * 2, torch.float64, -7.0)
    ub, u = canaried(n * K, torch.int32, -7)
    cb, c = canaried(n * 4, torch.int32, -7)
    scratch = torch.full((int(L().mkd_region_points_scratch_bytes(n)),), 0xA5, dtype=torch.uint8, device=DEV)          # (the call clears it itself)
    assert scratch.data_ptr() % 256 == 0 and m.data_ptr() % 256 == off % 256
    rc = L().mkd_region_points(P(m), n, H, W, dirs, min_area, P(p), P(u), P(c) if want_count else None, P(scratch), None)
    assert rc == 0, L().mkd_last_error()
    sync()
    pts, use = inside(pb, n * K * 2, -7.0, 'pts').reshape(n, K, 2), inside(ub, n * K, -7, 'use').reshape(n, K)
    cnt = inside(cb, n * 4, -7, 'count').reshape(n, 4)
    assert want_count or (cnt == -7).all()
    return pts, use, cnt


def coverage(H, W, n, seed):
    """name -> masks uint8 [4, n, H, W] (lip, skin, eye_left, eye_right); image b of a set is the set's picture rolled by b pixels"""
    rng = np.random.RandomState(seed)
    out = {}
    out['random'] = (rng.rand(4, n, H, W) < 0.3).astype(np.uint8) * rng.randint(1, 256, (4, n, H, W)).astype(np.uint8)
    out['dense'] = (rng.rand(4, n, H, W) < 0.9).astype(np.uint8) * 255
    out['nothing'] = np.zeros((4, n, H, W), dtype=np.uint8)
    full = np.ones((4, n, H, W), dtype=np.uint8)          # every mask full: the lip takes every pixel, the other three are empty
    out['every mask full'] = full
    # an empty lip, the skin over the whole image and over both eyes, a one-pixel eye in the last corner, an eye on the left border
    m = np.zeros((4, 1, H, W), dtype=np.uint8)
    m[1] = 3
    m[2, 0, H - 1, W - 1] = 1
    m[3, 0, 1:H - 1, 0] = 9
    out['full skin, one-pixel eye, border eye'] = m
    # rectangles (whole edges tie): the lip inside, an eye on the top border, an eye on the bottom border, the skin on the right border
    # and across the lip and the top eye
    m = np.zeros((4, 1, H, W), dtype=np.uint8)
    m[0, 0, H // 2:H // 2 + 3, 1:W - 2] = 1
    m[2, 0, 0:2, 2:W // 2] = 1
    m[3, 0, H - 2:H, W // 3:W - 1] = 1
    m[1, 0, 0:H - 1, W // 4:W] = 1
    out['rectangles on every border'] = m
    out['a face'] = pr.face_masks(H, W, (0.5, -0.5), 0.95, 12.0)[:, None]
    for name, m in list(out.items()):
        if m.shape[1] == 1:
            out[name] = np.concatenate([np.roll(m, (b, -b), (2, 3)) for b in range(n)], 1)
    return out


# ---- (a) the points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dirs', [8, 16])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_region_points_equal_the_restatement_byte_for_byte(shape, n, dirs):
    H, W = shape
    for i, (name, masks) in enumerate(coverage(H, W, n, 100 * H + 10 * n + dirs).items()):
        for min_area in ((1, 4) if i % 2 else (4, H * W // 3)):
            want = pr.region_points_ref(masks, dirs, min_area)
            got = run_points(masks, dirs, min_area, off=i % 4)
            for g, w, what in zip(got, want, ('pts', 'use', 'count')):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f'{name}, min_area {min_area}: {what}'
    # the picture of every case was looked at: regions do come out in use, and some do not
    _, use, cnt = pr.region_points_ref(coverage(H, W, n, 0)['rectangles on every border'], dirs, 4)
    assert use.any() and (cnt > 0).all()


def test_region_points_twice_without_count_and_through_the_wrapper():
    masks = coverage(64, 64, 3, 5)['a face']
    a, b = run_points(masks, 16, 4), run_points(masks, 16, 4, want_count=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    pts, use, count = teacher.region_points(torch.from_numpy(masks).to(DEV), 16, 4)
    assert (pts.dtype, use.dtype, count.dtype) == (torch.float64, torch.int32, torch.int32)
    assert tuple(pts.shape) == (3, 68, 2) and tuple(use.shape) == (3, 68) and tuple(count.shape) == (3, 4)
    for g, w in zip((pts, use, count), a):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        teacher.region_points(torch.from_numpy(masks).to(DEV), 12)
    with pytest.raises(ValueError):
        teacher.region_points(torch.from_numpy(masks[:3]).to(DEV))


# ---- (b) the solve -------------------------------------------------------------------------------------------------------------------
def run_solve(ps, pf, us=None, uf=None, M=None):
    """mkd_tps_solve, the outputs between canaries -> ctrl, coef, kcount numpy"""
    B, K, _ = ps.shape
    M = K if M is None else M
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    s, r, u, v = dev(ps, np.float64), dev(pf, np.float64), dev(us, np.int32), dev(uf, np.int32)
    cb, c = canaried(B * M * 2, torch.float64, -7.0)
    fb, f = canaried(B * 2 * (M + 3), torch.float64, -7.0)
    kb, k = canaried(B, torch.int32, -7)
    rc = L().mkd_tps_solve(P(s), P(r), P(u), P(v), B, K, M, P(c), P(f), P(k), None)
    assert rc == 0, L().mkd_last_error()
    sync()
    return (inside(cb, B * M * 2, -7.0, 'ctrl').reshape(B, M, 2), inside(fb, B * 2 * (M + 3), -7.0, 'coef').reshape(B, 2, M + 3),
            inside(kb, B, -7, 'kcount'))


def device_map(ctrl, coef, kcount, H, W):
    """the map of mkd_pgt_warp (map_out) for a spline given as numpy arrays -> float64 [B, 2, H, W]"""
    B = ctrl.shape[0]
    z = torch.zeros(B, 3, H, W, device=DEV)
    m = torch.zeros(4, B, H, W, dtype=torch.uint8, device=DEV)
    _, q = teacher.warp_blend(z, z, m, m, torch.from_numpy(ctrl).to(DEV), torch.from_numpy(coef).to(DEV), torch.from_numpy(kcount.astype(np.int32)).to(DEV),
                              torch.ones(B, 4, device=DEV), want_map=True)
    return q.cpu().numpy()


@pytest.fixture(scope='module')
def delta_ref():
    return pr.delta_ref()


@pytest.mark.parametrize('with_use', [False, True])
@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('case', [0, 1, 2])
def test_solve_against_the_host_solve(case, wide, with_use, delta_ref):
    name, H, W, ps, pf = pr.solve_cases()[case]
    B, K, _ = ps.shape
    M = 128 if wide else K
    us = uf = None
    if with_use and K > 3:
        rng = np.random.RandomState(K)
        us, uf = (rng.rand(B, K) < 0.85).astype(np.int32) * 5, (rng.rand(B, K) < 0.85).astype(np.int32)
    elif with_use:
        us, uf = np.ones((B, K), np.int32), np.full((B, K), -1, np.int32)          # any non-zero flag counts
    ctrl, coef, kcount = run_solve(ps, pf, us, uf, M)
    hc, hf, hk = np.zeros_like(ctrl), np.zeros_like(coef), np.zeros_like(kcount)
    for b in range(B):
        on = np.ones(K, bool) if us is None else (us[b] != 0) & (uf[b] != 0)
        c, f, k = teacher.tps_coefficients(ps[b][on][None], pf[b][on][None], max_ctrl=M)
        hc[b], hf[b], hk[b] = c[0], f[0], k[0]
        assert pr.full_residual(ctrl[b], coef[b], int(kcount[b]), pf[b][on]) <= pr.TPS_RESIDUAL
    assert ctrl.tobytes() == hc.tobytes() and kcount.tobytes() == hk.tobytes() and (hk >= 3).all()
    assert not coef[:, :, int(kcount.max()):M].any()
    diff = float(np.abs(device_map(ctrl, coef, kcount, H, W) - device_map(hc, hf, hk, H, W)).max())
    print(f'{name}, M = {M}, use {with_use}: map of the device solve against the host solve: max |diff| {diff:.3e} px; Delta_ref {delta_ref:.3e}')
    assert diff <= 16 * delta_ref
    again = run_solve(ps, pf, us, uf, M)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (ctrl, coef, kcount)))


def test_solve_on_mask_points_of_synthetic_faces(delta_ref):
    for H, W in ((64, 64), (40, 24)):
        ps, pf, us, uf = pr.paired_points(pr.face_pairs(H, W))
        ctrl, coef, kcount = run_solve(ps, pf, us, uf)
        want = pr.solve_ref(ps, pf, us, uf)
        assert ctrl.tobytes() == want[0].tobytes() and kcount.tobytes() == want[2].tobytes() and (kcount >= 3).all()
        for b in range(len(ps)):
            assert pr.full_residual(ctrl[b], coef[b], int(kcount[b]), pr.kept_pairs(ps[b], pf[b], us[b], uf[b])[1]) <= pr.TPS_RESIDUAL


def test_degenerate_samples():
    rng = np.random.RandomState(3)
    flat = rng.choice(32 * 32, 10, replace=False)
    base = np.stack([flat // 32, flat % 32], 1).astype(np.float64)
    line = np.stack([np.arange(2.0, 22.0, 2.0), np.zeros(10)], 1)          # x = 0
    nan, inf = base.copy(), base.copy()
    nan[3, 1], inf[0, 0] = np.nan, np.inf
    two = np.concatenate([base[:2]] * 5)
    rep = np.concatenate([base[:4], base[1:2], base[4:9], ])                # point 1 twice
    ones = np.ones(10, np.int32)
    off3 = ones.copy()
    off3[3] = 0
    few = np.zeros(10, np.int32)
    few[:2] = 1
    # (source, reference, use_src, use_ref) -> K_b
    samples = [(base, base + 1.0, ones, ones, 10), (line, line + 1.0, ones, ones, 0), (base, base - 1.0, ones, ones, 10),
               (nan, base, ones, ones, 0), (base, nan, ones, ones, 0), (base, inf, ones, ones, 0),
               (nan, base + 1.0, off3, ones, 9), (base, nan, ones, off3, 9),          # the NaN sits in a pair that is not in use
               (two, two, ones, ones, 0), (base, base, few, ones, 0), (base, base, ones, 0 * ones, 0),
               (rep, rep + rng.uniform(-2, 2, rep.shape), ones, ones, 9)]
    ps, pf = np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples])
    us, uf = np.stack([s[2] for s in samples]), np.stack([s[3] for s in samples])
    for M in (10, 128):
        ctrl, coef, kcount = run_solve(ps, pf, us, uf, M)
        assert kcount.tolist() == [s[4] for s in samples]
        want = pr.solve_ref(ps, pf, us, uf, M)
        assert ctrl.tobytes() == want[0].tobytes() and kcount.tobytes() == want[2].tobytes()
        for b, k in enumerate(kcount):
            if k == 0:
                assert not ctrl[b].any() and not coef[b].any()          # zeros everywhere, also between two good samples (1, between 0 and 2)
            else:
                assert pr.full_residual(ctrl[b], coef[b], int(k), pr.kept_pairs(ps[b], pf[b], us[b], uf[b])[1]) <= pr.TPS_RESIDUAL
        assert np.abs(coef[0, :, M] - 1.0).max() <= 1e-8 and np.abs(coef[2, :, M] + 1.0).max() <= 1e-8          # the translations
        assert np.array_equal(ctrl[11, :9], np.concatenate([base[:4], base[4:9]]))
        again = run_solve(ps, pf, us, uf, M)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (ctrl, coef, kcount)))
    got = teacher.tps_coefficients_device(torch.from_numpy(ps).to(DEV), torch.from_numpy(pf).to(DEV), torch.from_numpy(us).to(DEV),
                                          torch.from_numpy(uf).to(DEV), max_ctrl=128)
    assert all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(got, (ctrl, coef, kcount)))
    assert (got[0].dtype, got[1].dtype, got[2].dtype) == (torch.float64, torch.float64, torch.int32)


# ---- (c) pseudo_ground_truth(points=, solve=) ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pairs():
    src, ref, ss, rs = tr.synthetic_pairs()
    return (src, ref, ss, rs), tuple(torch.from_numpy(x).to(DEV) for x in (src, ref, ss, rs))


def packed_masks(ss, rs):
    return ms._region_masks_packed(torch.cat([ss, rs]), ms.LIP_CLASSES, ms.SKIN_CLASSES, ms.FACE_CLASSES, ms.EYE_LEFT_CLASSES, ms.EYE_RIGHT_CLASSES,
                                   ms.EYE_MARGIN)[0]


def bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize('feather,warp,dirs', [(2, True, 16), (0, {'eye': 1.0, 'lip': [0.0, 0.5, 1.0]}, 8)])
def test_mask_points_equal_the_chain_of_the_pieces(pairs, feather, warp, dirs):
    (src, ref, ss, rs), dev = pairs
    x_p, tables, counts = teacher.pseudo_ground_truth(*dev, feather=feather, warp=warp, points='masks', point_dirs=dirs)
    # masks -> tables -> compose (the alpha = 0 call) -> region_points -> tps_coefficients_device -> warp_blend
    xh, t0, c0 = teacher.pseudo_ground_truth(*dev, feather=feather)
    masks = packed_masks(dev[2], dev[3])
    pts, use, count = teacher.region_points(masks, dirs)
    ctrl, coef, kcount = teacher.tps_coefficients_device(pts[:3], pts[3:], use[:3], use[3:])
    want = teacher.warp_blend(xh, dev[1], masks[:, :3].contiguous(), masks[:, 3:].contiguous(), ctrl, coef, kcount, teacher.alpha_rows(warp, 3).to(DEV), feather)
    assert bits(x_p) == bits(want) and bits(tables) == bits(t0) and bits(counts) == bits(c0)
    assert bits(x_p) != bits(xh) and (kcount.cpu().numpy() >= 3).all()
    # the points are the restatement's on the restatement's masks, and the counts of the regions those of the histogram terms
    sm = tr.pseudo_ground_truth(src, ref, ss, rs, None, 0)[3]
    rm = tr.pseudo_ground_truth(ref, src, rs, ss, None, 0)[3]
    wp = pr.region_points_ref(np.concatenate([sm, rm], 1), dirs)
    assert all(bits(g) == w.tobytes() for g, w in zip((pts, use, count), wp))
    assert teacher.launches(warp=True, points='masks') == 21


def test_the_defaults_are_the_present_call_and_a_device_solve_is_its_chain(pairs, monkeypatch):
    _, dev = pairs
    rng = np.random.RandomState(8)
    flat = np.stack([rng.choice(32 * 32, 20, replace=False) for _ in range(3)])
    lms_s = np.stack([flat // 32, flat % 32], 2).astype(np.float32)
    lms_r = lms_s + rng.uniform(-2, 2, lms_s.shape).astype(np.float32)
    lms_s[2] = lms_s[2, :1]                                                # sample 2: one point twenty times -> no spline
    calls = []
    for name in ('region_points', 'tps_coefficients_device', 'tps_coefficients', 'warp_blend', 'compose'):
        inner = getattr(teacher, name)
        monkeypatch.setattr(teacher, name, lambda *a, _n=name, _f=inner, **k: (calls.append(_n), _f(*a, **k))[1])
    a = teacher.pseudo_ground_truth(*dev, lms_src=lms_s, lms_ref=lms_r, warp=True)
    first = list(calls)
    del calls[:]
    b = teacher.pseudo_ground_truth(*dev, lms_src=lms_s, lms_ref=lms_r, warp=True, points=None, point_dirs=16, solve='host')
    assert first == calls == ['tps_coefficients', 'compose', 'warp_blend'] and all(bits(x) == bits(y) for x, y in zip(a, b))
    assert teacher.launches(warp=True) == teacher.launches(warp=True, points=None, solve='host') == 17
    del calls[:]
    c = teacher.pseudo_ground_truth(*dev, lms_src=lms_s, lms_ref=torch.from_numpy(lms_r), warp=True, solve='device')
    assert calls == ['compose', 'tps_coefficients_device', 'warp_blend'] and teacher.launches(warp=True, solve='device') == 18
    xh = teacher.pseudo_ground_truth(*dev)[0]
    masks = packed_masks(dev[2], dev[3])
    ctrl, coef, kcount = teacher.tps_coefficients_device(torch.from_numpy(lms_s).double().to(DEV), torch.from_numpy(lms_r).double().to(DEV))
    want = teacher.warp_blend(xh, dev[1], masks[:, :3].contiguous(), masks[:, 3:].contiguous(), ctrl, coef, kcount, teacher.alpha_rows(True, 3).to(DEV), 2)
    assert bits(c[0]) == bits(want) and kcount.tolist() == [20, 20, 0]
    hc, hf, hk = teacher.tps_coefficients(lms_s, lms_r)
    assert bits(ctrl) == hc.tobytes() and bits(kcount) == hk.tobytes()
    # the device solve moves the image by no more than its map moves: 16 Delta_ref px at slope <= 4 per pixel, plus one fp32 rounding
    assert np.abs(c[0].cpu().numpy().astype(np.float64) - a[0].cpu().numpy()).max() <= 2.0 ** -23 + 4 * 16 * pr.delta_ref()
    assert bits(c[0][2]) == bits(xh[2]) == bits(a[0][2])
