"""-m gpu: mkd_noise_fill on the device against the numpy restatement (tests/noise_ref.py).  The raw words bit for bit on every tail
length, batch, row offset, sub-stream and both store forms; the normals within one fp32 ulp of the float64 restatement rounded once;
nothing written past n or past the last row; independence from the batch, the row slice and each of seed / sub / stream / row; the
moments at the host test's seed and bounds.

The launch count (one per call, whatever the shape) has no test: the library counts launches per context (mkd_step_launches*), and this
entry takes no context.  include/mkd.h and DESIGN.md section 0 state the count."""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_ref as nref
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import noise

pytestmark = pytest.mark.gpu

SEEDS = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1]          # both key words, and the sign bit of the int64 carrier
SUBS = [0, 1, 2 ** 31, 2 ** 32 - 1]
CANARY_U32 = 0x7FC0BEEF                                   # a NaN payload no normal and (with certainty 1 - 2^-32 per word) no word equals
STREAM = 2


def carrier(vals, bits):
    half, full = 1 << (bits - 1), 1 << bits
    return [v - full if v >= half else v for v in vals]


def fill(seeds, subs, stream, row0, rows, n, kind, offset=0, pad=8):
    """mkd_noise_fill into a canary-filled buffer with `pad` words before and after, the output starting `offset` words past a 16-byte
    boundary.  Returns (out [rows, B, n] int32 view of the bits, the words before, the words after)."""
    B = len(seeds)
    total = rows * B * n
    assert pad % 4 == 0
    buf = torch.full((pad + offset + total + pad,), CANARY_U32, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    s_dev = torch.tensor(carrier(seeds, 64), dtype=torch.int64, device=DEV)
    u_dev = None if subs is None else torch.tensor(carrier(subs, 32), dtype=torch.int32, device=DEV)
    out = buf[pad + offset:pad + offset + total]
    rc = L().mkd_noise_fill(P(s_dev), P(u_dev), B, stream, row0, rows, n, kind, P(out), None)
    assert rc == 0, L().mkd_last_error()
    sync()
    return out.view(rows, B, n), buf[:pad + offset], buf[pad + offset + total:]


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1. kind 1: the words ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 4, 5, 256, 1027])
@pytest.mark.parametrize('batch, rows', [(1, 1), (3, 10), (1, 10), (3, 1)])
def test_words_equal_the_restatement_bit_for_bit(n, batch, rows):
    for row0 in (0, 7):
        for subs in (None, SUBS[1:1 + batch]):
            seeds = (SEEDS + SEEDS)[row0 % 3:row0 % 3 + batch]
            ref = nref.fill(seeds, subs, STREAM, row0, rows, n, kind=1)
            vec, before, after = fill(seeds, subs, STREAM, row0, rows, n, 1, offset=0)
            assert np.array_equal(as_u32(vec), ref), (n, batch, rows, row0, subs)
            assert (before == CANARY_U32).all() and (after == CANARY_U32).all()
            # an `out` one float past the boundary: the scalar form, the same bits
            sca, before, after = fill(seeds, subs, STREAM, row0, rows, n, 1, offset=1)
            assert torch.equal(sca, vec)
            assert (before == CANARY_U32).all() and (after == CANARY_U32).all()


def test_every_seed_and_sub_word_reaches_the_key_and_the_counter():
    ref = nref.fill(SEEDS, SUBS, 5, 3, 2, 64, kind=1)
    out, _, _ = fill(SEEDS, SUBS, 5, 3, 2, 64, 1)
    assert np.array_equal(as_u32(out), ref)
    assert len({as_u32(out)[0, b].tobytes() for b in range(4)}) == 4
    # the python surface carries the same bits
    w = noise.words(SEEDS, (4, 4, 4), stream=5, rows=2, row0=3, subs=SUBS, device=DEV)
    assert tuple(w.shape) == (2, 4, 4, 4, 4) and np.array_equal(as_u32(w).reshape(2, 4, 64), ref)


# ---- 2. kind 0: the normals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, offset', [(1027, 0), (1024, 0), (1024, 1), (5, 3), (1 << 16, 0)])
def test_normals_within_one_ulp_of_the_restatement(n, offset):
    """The device evaluates log, sqrt and sincospi in double (each within a few double ulps) and rounds the product to fp32 ONCE; the
    restatement is accurate to a few double ulps too.  Two doubles that close round to the same fp32 unless a rounding boundary lies
    between them, in which case they round to NEIGHBOURS: the bound is one fp32 ulp, and the fraction of elements that differ at all
    is about 2^-53 / 2^-24 per double ulp of disagreement, some 1e-8 to 1e-7; the cap of 1 in 10^4 is a condition, not a measurement."""
    B, rows = (3, 4) if n < (1 << 16) else (1, 1)
    seeds = [11, 2 ** 64 - 1, 2 ** 32][:B]
    ref = nref.fill(seeds, None, nref.STREAM_ETA, 2, rows, n, kind=0).astype(np.float32)
    out, before, after = fill(seeds, None, nref.STREAM_ETA, 2, rows, n, 0, offset=offset)
    z = out.view(torch.float32).cpu().numpy()
    assert np.isfinite(z).all() and np.abs(z).max() <= np.float32(nref.Z_MAX)
    d = nref.ulp_distance(z, ref)
    differ = int((d != 0).sum())
    print(f'[noise] n {n} offset {offset}: max distance {int(d.max())} ulp, {differ} of {d.size} elements differ')
    assert d.max() <= 1
    assert differ * 10 ** 4 <= d.size
    # nothing beyond n or beyond the last row: the canaries around the output are whole
    assert (before == CANARY_U32).all() and (after == CANARY_U32).all()


def test_vector_and_scalar_forms_give_the_same_normals():
    a, _, _ = fill([5, 6], [0, 3], 0, 0, 3, 512, 0, offset=0)
    for off in (1, 2, 3):
        b, _, _ = fill([5, 6], [0, 3], 0, 0, 3, 512, 0, offset=off)
        assert torch.equal(a, b)
    assert torch.equal(noise.normal([5, 6], (512,), stream=0, rows=3, subs=[0, 3], device=DEV).view(torch.int32), a)


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch():
    full = noise.normal([0, 1, 2], (4, 8, 8), stream=noise.STREAM_START, device=DEV)
    rows = noise.normal([0, 1, 2], (4, 8, 8), stream=noise.STREAM_ETA, rows=10, device=DEV)
    assert tuple(full.shape) == (3, 4, 8, 8) and tuple(rows.shape) == (10, 3, 4, 8, 8) and full.dtype == torch.float32
    for b in range(3):
        assert torch.equal(noise.normal([b], (4, 8, 8), stream=noise.STREAM_START, device=DEV)[0], full[b])
        assert torch.equal(noise.normal([b], (4, 8, 8), stream=noise.STREAM_ETA, rows=10, device=DEV)[:, 0], rows[:, b])
    assert torch.equal(noise.normal([2, 0], (4, 8, 8), stream=noise.STREAM_START, device=DEV), full[[2, 0]])          # nor on its position


def test_a_row_slice_equals_the_rows_of_the_whole_call():
    whole = noise.normal([3, 9], (4, 8, 8), stream=noise.STREAM_BLEND, rows=10, device=DEV)
    assert torch.equal(noise.normal([3, 9], (4, 8, 8), stream=noise.STREAM_BLEND, rows=4, row0=5, device=DEV), whole[5:9])
    assert torch.equal(noise.normal([3, 9], (4, 8, 8), stream=noise.STREAM_BLEND, row0=7, device=DEV), whole[7])
    # the element index is the flat index of the per-sample shape: a reshape is the same noise
    assert torch.equal(noise.normal([3, 9], (256,), stream=noise.STREAM_BLEND, rows=10, device=DEV).view(10, 2, 4, 8, 8), whole)


def test_each_of_seed_sub_stream_and_row_changes_the_output():
    base = dict(seeds=[42], subs=[1], stream=16, row0=4)
    z0 = noise.normal(base['seeds'], (257,), stream=base['stream'], row0=base['row0'], subs=base['subs'], device=DEV)
    for change in (dict(seeds=[43]), dict(seeds=[42 + 2 ** 32]), dict(subs=[2]), dict(subs=[0]), dict(stream=17), dict(row0=5)):
        a = dict(base, **change)
        z = noise.normal(a['seeds'], (257,), stream=a['stream'], row0=a['row0'], subs=a['subs'], device=DEV)
        assert (z != z0).float().mean().item() > 0.99, change
    assert torch.equal(noise.normal([42], (257,), stream=16, row0=4, subs=None, device=DEV),
                       noise.normal([42], (257,), stream=16, row0=4, subs=[0], device=DEV))          # no subs: all 0


def test_the_torch_generators_are_not_advanced():
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    noise.normal([1, 2], (4, 8, 8), stream=0, rows=3, device=DEV)
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(DEV), dev)


# ---- 4. moments --------------------------------------------------------------------------------------------------------------------
def test_moments_of_the_device_normals():
    z = noise.normal([nref.MOMENT_SEED], (nref.MOMENT_N,), stream=noise.STREAM_START, device=DEV).cpu().numpy()
    mean, var, kurt = nref.moments(z)
    b_mean, b_var, b_kurt = nref.moment_bounds(nref.MOMENT_N)
    print(f'[moments] mean {mean:+.3e} (<= {b_mean:.3e}), var - 1 {var - 1:+.3e} (<= {b_var:.3e}), kurtosis - 3 {kurt - 3:+.3e} (<= {b_kurt:.3e})')
    assert abs(mean) <= b_mean and abs(var - 1.0) <= b_var and abs(kurt - 3.0) <= b_kurt
    assert np.abs(z).max() <= np.float32(nref.Z_MAX)


# ---- 5. capture --------------------------------------------------------------------------------------------------------------------
def test_the_fill_is_capturable():
    """no scratch, no host synchronisation: the launch records into a graph and replays to the same bits"""
    s_dev = torch.tensor([7, 8], dtype=torch.int64, device=DEV)
    out = torch.zeros(3, 2, 260, dtype=torch.float32, device=DEV)
    want = noise.normal([7, 8], (260,), stream=1, rows=3, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc = L().mkd_noise_fill(P(s_dev), None, 2, 1, 0, 3, 260, 0, P(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L().mkd_last_error()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    sync()
    assert torch.equal(out, want)
