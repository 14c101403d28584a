"""-m gpu: mkd_motion_warp against its restatement tests/motion_ref.py, bit for bit (integer arithmetic and copied bits: there is no
tolerance): the vectors, the warped pools, every slot named written and nothing else touched, every refusal before anything is
enqueued, and video.TemporalState with motion against the restated frame step."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as mr
import video_ref as vr
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import photo, video
from test_gpu_video import NAN_BITS, bits, dev, is_pattern, make_inputs, make_state, pattern, same_bits

pytestmark = pytest.mark.gpu

ERR_ARG = -1
# (n, S, block, search, penalty): one ragged block; ragged right and bottom; a search wider than the block with the halo clamped on all
# four sides, the largest batch; the narrowest search on a ragged tile of 8-blocks; one face, the widest search on 16-blocks; the
# smallest image in 8-blocks (three of a tile's four blocks lie outside it); the largest penalty and search: the largest costs (no
# vector can gain them: all zero)
CASES = [(1, 8, 16, 3, 0), (3, 24, 16, 2, 256), (16, 32, 8, 7, 0), (3, 40, 8, 1, 512), (1, 40, 16, 7, 100), (3, 8, 8, 7, 0), (1, 24, 16, 7, 65280)]
KINDS = ['random', 'shifted', 'ties', 'extremes']


def int_pattern(shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=DEV)


def make_slots(n, pool, seed):
    """permuted slots with every third face (from the second) without a previous frame; a single face has one"""
    rng = np.random.default_rng(seed)
    slot_in = rng.permutation(pool)[:n].tolist()
    for b in range(1, n, 3):
        slot_in[b] = -1
    return slot_in


def make_case(kind, n, S, search, pool, slot_in, seed):
    """s01 [n,3,S,S] and the previous state: random bytes with values at the rintf half-way points among them (make_inputs); the Y pool
    is, by kind, unrelated luminances, this frame's luminance displaced by a vector within the search (so the minimum is away from
    zero), the tie textures (a constant and a period of 2 in x, equal in both frames), or 65280 and 0 only.  Slots no face reads
    hold NaN."""
    rng = np.random.default_rng(seed)
    _, s01 = make_inputs(n, S, seed)
    dead = [s for s in range(pool) if s not in slot_in]
    D, Y = make_state(pool, S, seed + 1, dead)
    D.reshape(-1)[::97] = -0.0                                 # bits, not values, are copied
    for b, si in enumerate(slot_in):
        if si < 0:
            continue
        if kind == 'shifted':
            vy, vx = (int(v) for v in rng.integers(-search, search + 1, 2))
            Y[si] = np.roll(vr.luma(s01[b]), (vy, vx), (0, 1)).astype(np.float32)
        elif kind == 'ties':
            level = np.full((S, S), 97) if b % 2 else rng.integers(0, 200, (S, 1)) + 40 * (np.arange(S)[None] % 2)
            s01[b] = np.repeat((level.astype(np.float32) / np.float32(255.0))[None], 3, 0)
            Y[si] = vr.luma(s01[b]).astype(np.float32)
        elif kind == 'extremes':
            Y[si] = np.where(rng.random((S, S)) < 0.5, np.float32(65280.0), np.float32(0.0))
    return s01, D, Y


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,S,block,search,penalty', CASES)
def test_kernel_is_the_restatement_bit_for_bit(n, S, block, search, penalty, kind):
    pool = n + 3
    slot_in = [2] if n == 1 else make_slots(n, pool, 5 + S + search)
    s01, D_in, Y_in = make_case(kind, n, S, search, pool, slot_in, 200 + n + S + block + search)
    D_ref, Y_ref = np.zeros_like(D_in), np.zeros_like(Y_in)
    want = mr.pools_warp(s01, D_in, Y_in, slot_in, D_ref, Y_ref, search, block, penalty)
    if kind == 'ties':
        assert not want.any()
    if penalty == 65280:
        assert not want.any()
    elif kind == 'shifted':
        assert want.any()
    ms = video.MotionSearch(search, block, penalty)
    nb = -(-S // block)
    sd, Di, Yi = dev(s01), dev(D_in), dev(Y_in)
    D_w, Y_w, vec = pattern((pool, 3, S, S)), pattern((pool, S, S)), int_pattern((n, nb, nb, 2))
    assert video.motion_warp(sd, Di, Yi, slot_in, D_w, Y_w, ms, vec) is vec
    sync()
    got = vec.cpu().numpy()
    assert np.array_equal(got, want), f'{int((got != want).any(-1).sum())} of {n * nb * nb} vectors differ'
    for s in range(pool):
        if s in slot_in:
            assert same_bits(D_w[s], D_ref[s]) and same_bits(Y_w[s], Y_ref[s]), f'slot {s}'
        else:
            assert is_pattern(D_w[s]) and is_pattern(Y_w[s])          # slots not named keep their bytes
    assert same_bits(Di, D_in) and same_bits(Yi, Y_in) and same_bits(sd, s01)
    # without vec_out: the same pools
    D2, Y2 = pattern((pool, 3, S, S)), pattern((pool, S, S))
    assert video.motion_warp(sd, Di, Yi, slot_in, D2, Y2, ms) is None
    sync()
    assert torch.equal(bits(D2), bits(D_w)) and torch.equal(bits(Y2), bits(Y_w))


def test_a_single_face_without_a_previous_frame_touches_nothing():
    S = 24
    _, s01 = make_inputs(1, S, 9)
    D_in, Y_in = make_state(2, S, 10, dead=(0, 1))
    D_w, Y_w, vec = pattern((2, 3, S, S)), pattern((2, S, S)), int_pattern((1, 3, 3, 2))
    video.motion_warp(dev(s01), dev(D_in), dev(Y_in), [-1], D_w, Y_w, video.MotionSearch(3, 8, 0), vec)
    sync()
    assert is_pattern(D_w) and is_pattern(Y_w) and not vec.any()


def raw_call(s01, n, S, D_in, Y_in, slot_in, pool, search, block, penalty, D_w, Y_w, vec_out):
    arr = None if slot_in is None else (C.c_int32 * len(slot_in))(*slot_in)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return L().mkd_motion_warp(P(s01), n, S, P(D_in), P(Y_in), arr, pool, search, block, penalty, P(D_w), P(Y_w), P(vec_out), st)


def test_every_refusal_enqueues_nothing_and_a_valid_call_follows():
    n, S, pool = 2, 16, 4
    _, s01 = make_inputs(n, S, 1)
    D_in, Y_in = make_state(pool, S, 2)
    sd, Di, Yi = dev(s01), dev(D_in), dev(Y_in)
    both = pattern((2 * pool, 3, S, S))                   # one allocation: halves that do and do not overlap
    D_w, Y_w, vec = pattern((pool, 3, S, S)), pattern((pool, S, S)), int_pattern((n, 1, 1, 2))
    good = dict(s01=sd, n=n, S=S, D_in=Di, Y_in=Yi, slot_in=[1, -1], pool=pool, search=3, block=16, penalty=256, D_w=D_w, Y_w=Y_w, vec_out=vec)
    bad = [dict(s01=None), dict(D_in=None), dict(Y_in=None), dict(slot_in=None), dict(D_w=None), dict(Y_w=None),
           dict(n=0), dict(n=17, slot_in=[-1] * 17), dict(S=7), dict(S=1025), dict(search=0), dict(search=8), dict(search=-1),
           dict(block=4), dict(block=12), dict(block=32), dict(block=0), dict(penalty=-1), dict(penalty=65281), dict(pool=0), dict(pool=65537),
           dict(slot_in=[4, -1]), dict(slot_in=[1, -2]), dict(slot_in=[1, 1]), dict(slot_in=[3, 3]),
           dict(D_w=Di), dict(Y_w=Yi), dict(D_w=sd), dict(Y_w=sd), dict(D_w=Yi), dict(Y_w=Di), dict(Y_w=D_w[:, 0]),
           dict(D_in=both[:pool], D_w=both[pool - 1:2 * pool - 1])]
    for kw in bad:
        assert raw_call(**{**good, **kw}) == ERR_ARG, f'{list(kw)} was not refused'
    sync()
    assert is_pattern(D_w) and is_pattern(Y_w) and is_pattern(both) and bool((vec == NAN_BITS).all())
    assert same_bits(Di, D_in) and same_bits(Yi, Y_in) and same_bits(sd, s01)
    assert raw_call(**{**good, 'slot_in': [-1, -1]}) == 0                          # -1 may repeat
    assert raw_call(**{**good, 'D_in': both[:pool], 'D_w': both[pool:]}) == 0      # adjacent halves do not overlap
    assert raw_call(**good) == 0
    sync()
    D_ref, Y_ref = np.zeros_like(D_in), np.zeros_like(Y_in)
    want = mr.pools_warp(s01, D_in, Y_in, [1, -1], D_ref, Y_ref, 3, 16, 256)
    assert np.array_equal(vec.cpu().numpy(), want) and same_bits(D_w[1], D_ref[1]) and same_bits(Y_w[1], Y_ref[1])
    assert is_pattern(D_w[0]) and is_pattern(D_w[2:]) and is_pattern(Y_w[0]) and is_pattern(Y_w[2:])
    # the Python binding turns a refusal into an MkdError and checks shapes itself
    from makeupdiffuse_amd.lib import MkdError
    with pytest.raises(MkdError, match='must not repeat'):
        video.motion_warp(sd, Di, Yi, [2, 2], D_w, Y_w, video.MotionSearch())
    with pytest.raises(ValueError, match='pools hold the same number'):
        video.motion_warp(sd, Di, Yi, [1, -1], D_w[:2], Y_w, video.MotionSearch())
    with pytest.raises(ValueError, match='vec_out'):
        video.motion_warp(sd, Di, Yi, [1, -1], D_w, Y_w, video.MotionSearch(block=8), vec)
    with pytest.raises(ValueError, match='MotionSearch'):
        video.motion_warp(sd, Di, Yi, [1, -1], D_w, Y_w, (3, 16, 256))


def moving_faces(tracks, frames, S, seed):
    """per track a texture that moves by the track's own integer vector per frame, with a few bytes of change on top -> {(f, k): (t, s01)}"""
    rng = np.random.default_rng(seed)
    M = 3 * len(frames)
    out = {}
    for k in tracks:
        tex = rng.integers(0, 256, (3, S + 2 * M, S + 2 * M))
        vy, vx = (int(v) for v in rng.integers(-2, 3, 2))
        for f in range(len(frames)):
            win = tex[:, M + f * vy:M + f * vy + S, M + f * vx:M + f * vx + S] + (rng.random((3, S, S)) < 0.1) * rng.integers(0, 4, (3, S, S))
            s01 = (np.clip(win, 0, 255).astype(np.float32) / np.float32(255.0)).astype(np.float32)
            out[f, k] = (rng.uniform(-1.2, 1.2, (3, S, S)).astype(np.float32), s01)
    return out


@pytest.mark.parametrize('ms', [video.MotionSearch(2, 8, 64), None], ids=['motion', 'off'])
def test_three_frames_of_the_state_follow_the_restated_frame_step(ms):
    """video.TemporalState on the device (growing by reallocation in the second frame), faces that come, go and change order, against
    mr.frame_step on numpy pools led by a SlotPlan of their own: filtered samples, vectors and every slot named, bit for bit.  With
    motion=None the step is today's: no third pool, no vectors, one mkd_temporal_diff launch per frame."""
    S, filt = 20, video.TemporalFilter(0.8, 4.0, 1)
    frames = [[0, 1], [1, 0, 2], [2, 0]]
    data = moving_faces(range(3), frames, S, 13)
    state = video.TemporalState(filt, S, DEV, capacity=1, motion=ms)
    plan = video.SlotPlan()
    new = lambda: (np.zeros((8, 3, S, S), np.float32), np.zeros((8, S, S), np.float32))
    pin, pout, pw = new(), new(), new()
    moved = 0
    for f, ids in enumerate(frames):
        t, s01 = (np.stack([data[f, k][i] for k in ids]) for i in (0, 1))
        slot_in, slot_out = plan.assign(ids)
        want, vec = mr.frame_step(t, s01, pin[0], pin[1], slot_in, pw[0], pw[1], pout[0], pout[1], slot_out, tuple(filt), None if ms is None else tuple(ms))
        got = state.step(ids, dev(t), dev(s01), alive=len(ids))
        sync()
        assert same_bits(got, want), f'frame {f}'
        for so in slot_out:
            assert same_bits(state._in[0][so], pout[0][so]) and same_bits(state._in[1][so], pout[1][so])
        if ms is None:
            assert state.last_vectors is None and state._warp is None
        else:
            assert np.array_equal(state.last_vectors.cpu().numpy(), vec)
            moved += int(vec.any())
            for si in slot_in:
                assert si < 0 or (same_bits(state._warp[0][si], pw[0][si]) and same_bits(state._warp[1][si], pw[1][si]))
        pin, pout = pout, pin
    assert state.launches == 3 and state.capacity >= 3 and state.motion_launches == (0 if ms is None else 3)
    assert ms is None or moved >= 2                        # the clip does move: vectors away from zero were compared


def test_more_faces_than_a_launch_takes_are_split_into_chunks():
    S, n, ms = 8, photo.MAX_BATCH + 1, video.MotionSearch(1, 8, 0)
    filt = video.TemporalFilter(0.8, 4.0, 0)
    data = moving_faces(range(n), [0, 1], S, 14)
    state = video.TemporalState(filt, S, DEV, capacity=n, motion=ms)
    new = lambda: (np.zeros((n, 3, S, S), np.float32), np.zeros((n, S, S), np.float32))
    pin, pout, pw = new(), new(), new()
    ids = list(range(n))
    for f in range(2):
        t, s01 = (np.stack([data[f, k][i] for k in ids]) for i in (0, 1))
        want, vec = mr.frame_step(t, s01, pin[0], pin[1], [-1] * n if f == 0 else ids, pw[0], pw[1], pout[0], pout[1], ids, tuple(filt), tuple(ms))
        got = state.step(ids, dev(t), dev(s01), alive=n)
        sync()
        assert same_bits(got, want) and np.array_equal(state.last_vectors.cpu().numpy(), vec)
        pin, pout = pout, pin
    assert state.launches == 4 and state.motion_launches == 4
