"""-m gpu: mkd_temporal_diff against its restatement tests/video_ref.py, bit for bit (every value is a single-rounded fp32 expression or
an exact integer sum: there is no tolerance), every element written, nothing else touched, and every refusal before anything is
enqueued."""
import ctypes as C

import numpy as np
import pytest
import torch

import video_ref as vr
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import video

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0DEAD
ERR_ARG = -1
CASES = [(3, 16), (2, 20), (1, 8), (16, 16)]          # one tile; a ragged tile (halo and clamp meet); the smallest S; the largest batch


def pattern(shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(x):
    return x.contiguous().view(torch.int32)


def is_pattern(x):
    return bool((bits(x) == NAN_BITS).all())


def make_inputs(n, S, seed):
    """s01 from bytes / 255 with 0 and 255 among them and values whose product with 255 lies within an ulp of a tie; t in [-1.2, 1.2]"""
    rng = np.random.default_rng(seed)
    s01 = (rng.integers(0, 256, (n, 3, S, S)).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    flat = s01.reshape(-1)
    flat[0], flat[1], flat[-1] = 0.0, 1.0, 1.0
    ties = ((rng.integers(0, 255, 24).astype(np.float32) + np.float32(0.5)) / np.float32(255.0)).astype(np.float32)
    ties = np.concatenate([ties[:8], np.nextafter(ties[8:16], np.float32(2.0)), np.nextafter(ties[16:], np.float32(-1.0))]).astype(np.float32)
    flat[rng.choice(flat.size - 3, ties.size, replace=False) + 2] = ties
    t = rng.uniform(-1.2, 1.2, (n, 3, S, S)).astype(np.float32)
    return t, s01


def make_state(pool, S, seed, dead=()):
    """a plausible previous frame in every slot; the slots ``dead`` hold NaN"""
    rng = np.random.default_rng(seed)
    D = rng.uniform(-0.5, 0.5, (pool, 3, S, S)).astype(np.float32)
    Y = np.stack([vr.luma(rng.integers(0, 256, (3, S, S)).astype(np.float32) / np.float32(255.0)) for _ in range(pool)]).astype(np.float32)
    for s in dead:
        D[s], Y[s] = np.nan, np.nan
    return D, Y


def make_slots(n, pool, seed):
    rng = np.random.default_rng(seed)
    slot_out = rng.permutation(pool)[:n].tolist()
    slot_in = rng.permutation(pool)[:n].tolist()
    for b in range(0, n, 3):          # a mix of faces without a previous frame and faces with one, in shuffled order
        slot_in[b] = -1
    if n == 1:
        slot_in = [int(rng.integers(0, pool))]
    return slot_in, slot_out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    return torch.equal(bits(got).cpu(), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))


@pytest.mark.parametrize('radius', [0, 1, 2])
@pytest.mark.parametrize('n,S', CASES)
def test_kernel_is_the_restatement_bit_for_bit(n, S, radius):
    filt = video.TemporalFilter(0.8, 4.0, radius)
    pool = n + 3
    t, s01 = make_inputs(n, S, 100 + n + S)
    if n == 1:          # the single face once with a previous frame and once without
        variants = [make_slots(n, pool, 7 + S + radius), ([-1], [2])]
    else:
        variants = [make_slots(n, pool, 7 + S + radius)]
    for slot_in, slot_out in variants:
        dead = [s for s in range(pool) if s not in slot_in]          # no face reads these: NaN there must not reach an output
        D_in, Y_in = make_state(pool, S, 3 + S, dead)
        D_ref, Y_ref = np.zeros_like(D_in), np.zeros_like(Y_in)
        want = vr.pools_step(t, s01, D_in, Y_in, slot_in, D_ref, Y_ref, slot_out, filt.beta, filt.tau, radius)
        td, sd = dev(t), dev(s01)
        D_out, Y_out, out = pattern((pool, 3, S, S)), pattern((pool, S, S)), pattern((n, 3, S, S))
        got = video.temporal_diff(td, sd, dev(D_in), dev(Y_in), slot_in, D_out, Y_out, slot_out, filt, out=out)
        sync()
        assert got is out and torch.isfinite(out).all()
        assert same_bits(out, want), f'{int((bits(out).cpu() != torch.from_numpy(want).view(torch.int32)).sum())} elements of t_out differ'
        for b in range(n):
            so = slot_out[b]
            assert torch.isfinite(D_out[so]).all() and torch.isfinite(Y_out[so]).all()
            assert same_bits(D_out[so], D_ref[so]) and same_bits(Y_out[so], Y_ref[so])
            if slot_in[b] < 0:
                assert same_bits(out[b], t[b])                   # the bits of t
        for s in range(pool):
            if s not in slot_out:
                assert is_pattern(D_out[s]) and is_pattern(Y_out[s])          # slots not named keep their bytes
        # t_out aliasing t gives the same bits
        alias = td.clone()
        D2, Y2 = pattern((pool, 3, S, S)), pattern((pool, S, S))
        assert video.temporal_diff(alias, sd, dev(D_in), dev(Y_in), slot_in, D2, Y2, slot_out, filt, out=alias) is alias
        sync()
        assert torch.equal(bits(alias), bits(out)) and torch.equal(bits(D2), bits(D_out)) and torch.equal(bits(Y2), bits(Y_out))


def test_three_frames_of_ping_pong_follow_three_steps_of_the_restatement():
    """video.TemporalState on the device: faces come and go and change order; every track against its own chain of vr.step"""
    S, filt = 20, video.TemporalFilter(0.8, 4.0, 1)
    state = video.TemporalState(filt, S, DEV, capacity=1)          # (grows by reallocation in the second frame, keeping what it holds)
    frames = [[0, 1], [1, 0, 2], [2, 0], [0, 2, 1]]
    rng = np.random.default_rng(11)
    base = {k: make_inputs(1, S, 40 + k) for k in range(3)}
    chain = {}
    for f, ids in enumerate(frames):
        t = np.stack([base[k][0][0] + np.float32(0.01 * f) for k in ids]).astype(np.float32)
        s01 = np.stack([np.clip(base[k][1][0] + np.float32(f * 3 / 255.0) * (rng.random((3, S, S)) < 0.3), 0, 1) for k in ids]).astype(np.float32)
        got = state.step(ids, dev(t), dev(s01), alive=len(ids))
        sync()
        for j, k in enumerate(ids):
            prev = chain.get(k, (None, None)) if f == 0 or k in frames[f - 1] else (None, None)          # a face that was away starts over
            want, D, Y = vr.step(t[j], s01[j], prev[0], prev[1], filt.beta, filt.tau, filt.radius)
            chain[k] = (D, Y)
            assert same_bits(got[j], want), f'frame {f}, track {k}'
            assert same_bits(state._in[0][state.plan.held[k]], D) and same_bits(state._in[1][state.plan.held[k]], Y)
    assert state.launches == 4 and state.capacity >= 3


def raw_call(t, s01, n, S, D_in, Y_in, slot_in, D_out, Y_out, slot_out, pool, beta, tau, radius, t_out):
    arr = lambda v: None if v is None else (C.c_int32 * len(v))(*v)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return L().mkd_temporal_diff(P(t), P(s01), n, S, P(D_in), P(Y_in), arr(slot_in), P(D_out), P(Y_out), arr(slot_out), pool, beta, tau, radius,
                                 P(t_out), st)


def test_every_refusal_enqueues_nothing_and_a_valid_call_follows():
    n, S, pool = 2, 16, 4
    t, s01 = make_inputs(n, S, 1)
    D_in, Y_in = make_state(pool, S, 2)
    td, sd, Di, Yi = dev(t), dev(s01), dev(D_in), dev(Y_in)
    both = pattern((2 * pool, 3, S, S))                   # one allocation: halves that do and do not overlap
    D_out, Y_out, out = pattern((pool, 3, S, S)), pattern((pool, S, S)), pattern((n, 3, S, S))
    good = dict(t=td, s01=sd, n=n, S=S, D_in=Di, Y_in=Yi, slot_in=[1, -1], D_out=D_out, Y_out=Y_out, slot_out=[3, 0], pool=pool, beta=0.8, tau=4.0,
                radius=1, t_out=out)
    bad = [dict(t=None), dict(s01=None), dict(D_in=None), dict(Y_in=None), dict(slot_in=None), dict(D_out=None), dict(Y_out=None),
           dict(slot_out=None), dict(t_out=None),
           dict(n=0), dict(n=17, slot_in=[-1] * 17, slot_out=list(range(17)), pool=32), dict(S=7), dict(S=1025), dict(radius=-1), dict(radius=3),
           dict(beta=0.0), dict(beta=-0.5), dict(beta=0.96), dict(beta=float('nan')),
           dict(tau=0.4), dict(tau=2e6), dict(tau=float('inf')), dict(tau=float('nan')),
           dict(slot_in=[4, -1]), dict(slot_in=[1, -2]), dict(slot_out=[4, 0]), dict(slot_out=[-1, 0]), dict(slot_out=[3, 3]), dict(pool=0),
           dict(D_out=Di), dict(Y_out=Yi), dict(D_in=both[:pool], D_out=both[pool - 1:2 * pool - 1]), dict(Y_out=D_out[:, 0])]
    for kw in bad:
        assert raw_call(**{**good, **kw}) == ERR_ARG, f'{list(kw)} was not refused'
    sync()
    assert is_pattern(D_out) and is_pattern(Y_out) and is_pattern(out) and is_pattern(both)
    assert torch.equal(bits(Di).cpu(), torch.from_numpy(D_in).view(torch.int32)) and torch.equal(bits(Yi).cpu(), torch.from_numpy(Y_in).view(torch.int32))
    assert raw_call(**{**good, 'D_in': both[:pool], 'D_out': both[pool:]}) == 0          # adjacent halves do not overlap
    assert raw_call(**good) == 0
    sync()
    D_ref, Y_ref = np.zeros_like(D_in), np.zeros_like(Y_in)
    want = vr.pools_step(t, s01, D_in, Y_in, [1, -1], D_ref, Y_ref, [3, 0], 0.8, 4.0, 1)
    assert same_bits(out, want) and same_bits(D_out[3], D_ref[3]) and same_bits(D_out[0], D_ref[0]) and same_bits(Y_out[3], Y_ref[3])
    assert is_pattern(D_out[1:3]) and is_pattern(Y_out[1:3])
    # the Python binding turns a refusal into an MkdError and checks shapes itself
    from makeupdiffuse_amd.lib import MkdError
    with pytest.raises(MkdError, match='slot_out must not repeat'):
        video.temporal_diff(td, sd, Di, Yi, [1, -1], D_out, Y_out, [2, 2], video.TemporalFilter())
    with pytest.raises(ValueError, match='pools hold the same number'):
        video.temporal_diff(td, sd, Di, Yi, [1, -1], D_out[:2], Y_out, [1, 0], video.TemporalFilter())
