"""Video clips, the host side (no device): video.FaceTracker, video.smooth_frame, the validated TemporalFilter and the slot plan of its
state, and the properties of the temporal filter on the numpy restatement tests/video_ref.py (the lines of include/mkd.h
mkd_temporal_diff) followed by the paste restatement tests/photo_ref.py."""
import math

import numpy as np
import pytest

import photo_ref as pr
import video_ref as vr
from makeupdiffuse_amd import photo, video

F32 = np.float32


def sq(cx, cy, side):
    """the integer square box centred at (cx, cy)"""
    return (int(cx - side // 2), int(cy - side // 2), int(side), int(side))


# ---- tracker ------------------------------------------------------------------------------------------------------------------------
def test_two_faces_that_swap_detection_order_keep_their_ids():
    tr = video.FaceTracker()
    a, b = sq(40, 40, 30), sq(120, 50, 28)
    assert tr.update([a, b]) == [0, 1] and tr.restarted == [True, True]
    assert tr.update([sq(122, 51, 31), sq(41, 40, 29)]) == [1, 0] and tr.restarted == [False, False]          # b grew past a: found first
    assert tr.update([sq(42, 41, 29), sq(123, 51, 31)]) == [0, 1]
    assert tr.alive == [0, 1] and tr.next_id == 2


def test_a_face_back_within_max_gap_keeps_its_id_and_restarts():
    tr = video.FaceTracker(max_gap=3)
    a, b = sq(40, 40, 30), sq(120, 50, 28)
    assert tr.update([a, b]) == [0, 1]
    for _ in range(3):                                   # b is away for max_gap frames
        assert tr.update([a]) == [0] and tr.restarted == [False]
    assert tr.alive == [0, 1]
    assert tr.update([a, b]) == [0, 1] and tr.restarted == [False, True]          # the same id (the same noise), a fresh temporal state
    assert tr.update([a, b]) == [0, 1] and tr.restarted == [False, False]
    # ... and the slot plan of the filter's state follows the flag: no previous slot for the face that was away
    plan = video.SlotPlan()
    assert plan.assign([0, 1]) == ([-1, -1], [0, 1])
    assert plan.assign([1, 0]) == ([1, 0], [0, 1])                                # each reads what IT wrote, whatever the order
    assert plan.assign([0]) == ([1], [0])
    assert plan.assign([0, 1], [False, True]) == ([0, -1], [0, 1])
    assert plan.assign([0, 1], [False, False]) == ([0, 1], [0, 1])
    assert plan.assign([]) == ([], []) and plan.assign([0]) == ([-1], [0])       # a frame without a face drops every state
    with pytest.raises(ValueError, match='once per frame'):
        plan.assign([2, 2])


def test_a_face_back_after_more_than_max_gap_is_a_new_track():
    tr = video.FaceTracker(max_gap=2)
    a, b = sq(40, 40, 30), sq(120, 50, 28)
    assert tr.update([a, b]) == [0, 1]
    for _ in range(3):
        assert tr.update([a]) == [0]
    assert tr.alive == [0]
    assert tr.update([a, b]) == [0, 2] and tr.restarted == [False, True]          # ids are never used again


def test_a_jump_or_a_scale_change_beyond_the_limits_starts_a_new_track():
    tr = video.FaceTracker(max_jump=0.5, max_scale=1.5)
    assert tr.update([sq(50, 50, 40)]) == [0]
    assert tr.update([sq(70, 50, 40)]) == [0]                                      # 20 / 40 = 0.5: still the track
    assert tr.update([sq(91, 50, 40)]) == [1]                                      # 21 / 40 > 0.5, measured from the last RAW detection
    assert tr.update([sq(91, 50, 62)]) == [2] and tr.alive == [0, 1, 2]            # 62 / 40 > 1.5
    assert tr.update([photo.frame_from_box(sq(91, 50, 60), 20.0)]) == [1]          # a Frame is normalised like a box; 60 / 40 = 1.5


def test_ties_go_to_the_lowest_id():
    tr = video.FaceTracker(max_jump=1.0)
    assert tr.update([sq(40, 50, 20), sq(80, 50, 20)]) == [0, 1]
    assert tr.update([sq(60, 50, 20)]) == [0]                                      # both at 20 / 20: the lowest id
    tr = video.FaceTracker(max_jump=1.0)
    assert tr.update([sq(80, 50, 20), sq(40, 50, 20)]) == [0, 1]
    assert tr.update([sq(60, 50, 20)]) == [0]
    assert tr.update([sq(60, 50, 20), sq(59, 50, 20)]) == [0, 1]                   # a taken track is no candidate


def clip_faces():
    """8 frames: two faces that drift, swap order at frame 3, one of them away in frames 5 and 6"""
    out = []
    for f in range(8):
        a, b = sq(40 + 2 * f, 40 + f, 30 + (f % 2) * 2), sq(120 - f, 52, 26 + 2 * f)
        fl = [a, b] if f < 3 else [b, a]
        out.append([fl[0]] if f in (5, 6) else fl)
    return out


def run_host(split, gamma=0.5):
    tr, hat, ids, regions, rest = video.FaceTracker(), {}, [], [], []
    clip, f0 = clip_faces(), 0
    for n in split:                                       # what VideoSession does per push, frame by frame
        for fl in clip[f0:f0 + n]:
            got = tr.update(fl)
            regs = []
            for tid, fresh, raw in zip(got, tr.restarted, fl):
                hat[tid] = video.smooth_frame(None if fresh else hat.get(tid), raw, gamma)
                regs.append(hat[tid])
            for tid in [k for k in hat if k not in got]:
                del hat[tid]
            ids.append(got)
            regions.append(regs)
            rest.append(list(tr.restarted))
        f0 += n
    return ids, regions, rest


def test_host_decisions_do_not_depend_on_the_split_into_pushes():
    want = run_host((8,))
    assert want[0][2] == [0, 1] and want[0][3] == [1, 0] and want[0][7] == [1, 0] and want[2][7] == [False, True]
    for split in ((1, 7), (4, 4), (3, 3, 2)):
        assert run_host(split) == want


def test_video_session_follows_the_same_host_decisions():
    """VideoSession._track is the loop above (the model and the device are not needed for it)"""
    s = video.VideoSession.__new__(video.VideoSession)
    s.tracker, s._hat, s.gamma = video.FaceTracker(), {}, 0.5
    got = [s._track(fl) for fl in clip_faces()]
    want = run_host((8,))
    assert [g[0] for g in got] == want[0] and [g[2] for g in got] == want[1] and [g[1] for g in got] == want[2]


# ---- smoothing ----------------------------------------------------------------------------------------------------------------------
def test_first_frame_is_the_raw_frame_and_gamma_0_the_identity():
    box, fr = (10, 20, 40, 40), photo.frame_from_box((10, 20, 40, 40), 12.0)
    assert video.smooth_frame(None, box, 0.5) is box and video.smooth_frame(None, fr, 0.5) is fr
    assert video.smooth_frame((0, 0, 50, 50), box, 0.0) is box                     # the caller's integer box: the crop_resize / paste_photos calls
    assert video.smooth_frame(photo.frame_from_box((0, 0, 50, 50), 30.0), fr, 0) is fr
    for bad in (-0.1, 0.96, math.nan, 'x', True):
        with pytest.raises(ValueError, match='box_smooth'):
            video.smooth_frame(None, box, bad)
    with pytest.raises(ValueError, match='not square'):
        video.smooth_frame((0, 0, 50, 50), (0, 0, 50, 40), 0.5)


def test_smoothing_is_the_recursion_on_centre_log_side_and_angle():
    prev, cur = photo.frame_from_box((10, 20, 40, 40), 10.0), photo.frame_from_box((14, 26, 50, 50), 30.0)
    g = 0.25
    got = video.smooth_frame(prev, cur, g)
    assert isinstance(got, photo.Frame)
    assert got.cx == pytest.approx(39 + g * (30 - 39), abs=1e-12) and got.cy == pytest.approx(51 + g * (40 - 51), abs=1e-12)
    assert got.side == pytest.approx(math.exp(math.log(50) + g * (math.log(40) - math.log(50))), rel=1e-14)
    assert math.degrees(math.atan2(got.s, got.c)) == pytest.approx(30 + g * (10 - 30), abs=1e-10)
    assert abs(got.c ** 2 + got.s ** 2 - 1) < 1e-12
    photo.check_frame(got, 200, 200, 64)


def test_the_angle_wraps_across_180_degrees():
    prev, cur = photo.frame_from_box((10, 10, 40, 40), 170.0), photo.frame_from_box((10, 10, 40, 40), -170.0)
    got = video.smooth_frame(prev, cur, 0.5)                                       # 20 degrees apart across the cut: half way is 180, not 0
    assert abs(abs(math.degrees(math.atan2(got.s, got.c))) - 180.0) < 1e-9
    got = video.smooth_frame(cur, prev, 0.25)
    assert math.degrees(math.atan2(got.s, got.c)) == pytest.approx(175.0, abs=1e-9)
    assert video._wrap180(180.0) == 180.0 and video._wrap180(-180.0) == 180.0 and video._wrap180(540.0) == 180.0 and video._wrap180(-190.0) == 170.0


def test_a_constant_input_is_a_fixed_point_bit_for_bit():
    for cur in ((11, 23, 47, 47), photo.frame_from_box((11, 23, 47, 47), 33.3), photo.Frame(40.3, 51.7, 33.1, math.cos(0.7), math.sin(0.7))):
        hat = video.smooth_frame(None, cur, 0.7)
        for _ in range(5):
            hat = video.smooth_frame(hat, cur, 0.7)
            want = photo.frame_from_box(cur) if len(cur) == 4 else cur
            assert tuple(hat) == tuple(want)                                       # == on floats: the bits (no -0.0 among them)
    for box in ((11, 23, 47, 47), (10, 22, 48, 48)):          # a still face keeps taking the axis-aligned calls
        assert photo.box_from_frame(video.smooth_frame(box, box, 0.7)) == box


# ---- the validated filter -----------------------------------------------------------------------------------------------------------
def test_temporal_filter_is_validated():
    assert tuple(video.TemporalFilter()) == (0.8, 4.0, 1) and video.TemporalFilter(0.95, 0.5, 2).radius == 2
    for kw in (dict(beta=0.0), dict(beta=0.96), dict(beta=math.nan), dict(beta='a'), dict(tau=0.4), dict(tau=math.inf), dict(tau=2e6),
               dict(radius=3), dict(radius=-1), dict(radius=1.0), dict(radius=True)):
        with pytest.raises(ValueError, match='TemporalFilter'):
            video.TemporalFilter(**kw)


# ---- the filter's restatement -------------------------------------------------------------------------------------------------------
S = 16
BOX, HW = (3, 2, 37, 41), (48, 44)


def bytes01(rng, shape=(3, S, S)):
    return (rng.integers(0, 256, shape).astype(F32) / F32(255.0)).astype(F32)


def test_steady_clip_is_unfiltered_bit_for_bit_and_pastes_equal_bytes():
    rng = np.random.default_rng(5)
    s01, t = bytes01(rng), rng.uniform(-1.2, 1.2, (3, S, S)).astype(F32)
    photo_u8 = rng.integers(0, 256, HW + (3,)).astype(np.uint8)
    d = vr.diff(t, s01)
    outs, Ds = vr.run([t] * 6, [s01] * 6, beta=0.8, tau=4.0, radius=1)
    first = pr.paste(photo_u8, BOX, outs[0], s01, 3)
    assert np.array_equal(outs[0].view(np.uint32), t.view(np.uint32))
    for o, D in zip(outs, Ds):
        assert np.array_equal(D.view(np.uint32), d.view(np.uint32))               # k * 0 = 0: D = d on every frame
        assert np.array_equal(pr.paste(photo_u8, BOX, o, s01, 3), first)
    assert (first != photo_u8).any()


def test_noise_falls_to_a_third():
    rng = np.random.default_rng(2024)
    s01 = bytes01(np.random.default_rng(6))
    T, burn, beta = 256, 32, 0.8
    d = (0.1 + 0.02 * rng.standard_normal((T, 3, S, S))).astype(F32)
    ts = [((s01 + d[i]) * F32(2.0) - F32(1.0)).astype(F32) for i in range(T)]
    _, Ds = vr.run(ts, [s01] * T, beta=beta, tau=4.0, radius=1)
    std_in = np.stack([vr.diff(t, s01) for t in ts])[burn:].std(axis=0).mean()
    std_out = np.stack(Ds)[burn:].std(axis=0).mean()
    ratio = float(std_out / std_in)
    want = math.sqrt((1 - beta) / (1 + beta))
    assert want == pytest.approx(1 / 3)
    print(f'temporal std ratio {ratio:.4f}, sqrt((1 - beta) / (1 + beta)) = {want:.4f}')
    assert abs(ratio - want) <= 0.1 * want                # the sampling error of 224 correlated frames, not an accuracy of the code


def test_a_scene_cut_restarts_the_filter():
    """every pixel's luminance moves by L = 100 levels: A = N 256 L, q = L / tau = 25 exactly, c = 1 / 626, k = beta / 626 = 1.278e-3"""
    rng = np.random.default_rng(7)
    g0 = rng.integers(0, 120, (S, S))
    s_a = np.repeat((g0.astype(F32) / F32(255.0))[None], 3, 0)                    # grey frames: Y = 256 x the level
    s_b = np.repeat(((g0 + 100).astype(F32) / F32(255.0))[None], 3, 0)
    assert np.array_equal(vr.luma(s_b) - vr.luma(s_a), np.full((S, S), 25600))
    k = vr.gain(vr.luma(s_b), vr.luma(s_a).astype(F32), 0.8, 4.0, 1)
    bound = 0.8 / (1.0 + 25.0 ** 2)
    assert bound == pytest.approx(1.278e-3, rel=1e-3)
    assert np.all(k <= F32(bound) * (1 + 2.0 ** -22)) and np.all(k > 0)
    d_old, d_new = F32(0.3), F32(-0.2)
    t_a = ((s_a + d_old) * F32(2.0) - F32(1.0)).astype(F32)
    t_b = ((s_b + d_new) * F32(2.0) - F32(1.0)).astype(F32)
    _, Ds = vr.run([t_a, t_a, t_b], [s_a, s_a, s_b], beta=0.8, tau=4.0, radius=1)
    new = vr.diff(t_b, s_b)
    survives = np.abs(Ds[2] - new) / np.abs(Ds[1] - new)                           # the share of (old - new) left in the output
    assert float(survives.max()) <= bound * (1 + 1e-3) + 2.0 ** -20                # fp32 rounding of D on top of the derived bound


def test_a_local_change_lowers_the_gain_only_within_the_radius():
    rng = np.random.default_rng(8)
    s_a = bytes01(rng, (3, 24, 24))
    s_b = s_a.copy()
    s_b[:, 9:13, 10:14] = (F32(1.0) - s_a[:, 9:13, 10:14]).astype(F32)           # one 4 x 4 block changes
    changed = vr.luma(s_b) != vr.luma(s_a)
    assert changed[9:13, 10:14].any() and not changed[:9].any() and not changed[:, 14:].any()
    for R in (0, 1, 2):
        k = vr.gain(vr.luma(s_b), vr.luma(s_a).astype(F32), 0.8, 4.0, R)
        near = np.zeros((24, 24), bool)
        near[9 - R:13 + R, 10 - R:14 + R] = True
        assert np.all(k[~near] == F32(0.8)) and np.all(k[near] <= F32(0.8))
        reach = vr.window_sum(changed.astype(np.int64), R) > 0
        assert np.all(k[reach] < F32(0.8)) and not reach[~near].any()
