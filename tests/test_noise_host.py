"""CPU: the counter-based noise without a device.  The numpy restatement (tests/noise_ref.py) against Random123's known answers, the
uniform's exactness, the bound on |z|, the moments of the reference at the seed the device test reuses, as_seeds' validation, every
refusal of mkd_noise_fill that needs no device, and the seeds / x_T argument rules of the samplers, the model and runs/test.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_ref as nref
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import noise
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.diffmk.makeup_diffuse import DiagonalGaussianPosterior, TestDiffuseModel
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler
from makeupdiffuse_amd.unipc import UniPCSampler
from test_dpm_solver_host import HostModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ctr, key, want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_reproduces_the_random123_known_answers(ctr, key, want):
    got = nref.philox4x32_10(np.asarray(ctr, dtype=np.uint64), np.asarray(key, dtype=np.uint64))
    assert tuple(int(v) for v in got) == want


def test_counter_and_key_layout():
    """block j of (seed, sub, stream, row) is Philox of the counter (j, row, stream, sub) under the key (seed low, seed high)"""
    seed, sub, stream, row = 0x299f31d0a4093822, 0x03707344, 0x13198a2e, 0x85a308d3
    q = nref.blocks(seed, sub, stream, row, 4 * (0x2a + 1))
    want = nref.philox4x32_10(np.asarray([0x2a, row, stream, sub], dtype=np.uint64), np.asarray([0xa4093822, 0x299f31d0], dtype=np.uint64))
    assert np.array_equal(q[0x2a], want)
    assert nref.fill([seed], [sub], stream, row, 1, 7, kind=1).shape == (1, 1, 7)
    assert np.array_equal(nref.fill([seed], [sub], stream, row, 1, 7, kind=1)[0, 0], q.reshape(-1)[:7])


def test_uniform_is_exact_and_open():
    for w, num in ((0, 1), (0xff, 1), (0x100, 3), (0xffffffff, (1 << 25) - 1)):
        u = float(nref.unit(np.uint32(w)))
        assert u == num / 2.0 ** 25 and 0.0 < u < 1.0          # ((w >> 8) + 0.5) 2^-24 = (2 (w >> 8) + 1) 2^-25
        assert u * 2.0 ** 25 == num and float(u * 2.0 ** 25).is_integer()          # the rational itself: nothing was rounded
    # an odd numerator of up to 25 bits: exact in double, and in fp32 only below a half -- fp32 would round the largest u to 1, which is
    # one reason the definition evaluates in double
    assert float(nref.unit(np.uint32(0xffffffff))) == 1.0 - 2.0 ** -25 and float(np.float32(1.0 - 2.0 ** -25)) == 1.0
    assert float(np.float32(nref.unit(np.uint32(0x7fffffff)))) == float(nref.unit(np.uint32(0x7fffffff)))


def test_exact_angle_folding_agrees_with_the_plain_evaluation():
    g = np.random.default_rng(5)
    w = g.integers(0, 1 << 32, size=1 << 14, dtype=np.uint64)
    c, s = nref.cos_sin_turn(w)
    ang = 2.0 * np.pi * nref.unit(w)
    assert np.abs(c - np.cos(ang)).max() < 1e-15 and np.abs(s - np.sin(ang)).max() < 1e-15
    assert np.abs(c * c + s * s - 1.0).max() < 1e-15
    # next to the zeros of cos and sin the folded form keeps the sign and the size: a quarter turn + 2^-25 turns
    for turn_q in (1, 3):
        m = turn_q * (1 << 23) + 1
        c, _ = nref.cos_sin_turn(np.uint64((m - 1) // 2 << 8))
        tiny = np.sin(2.0 * np.pi / 2.0 ** 25)          # (= the angle less its cube over six, 1.1e-21)
        assert np.sign(c) == (-1 if turn_q == 1 else 1) and abs(abs(c) - tiny) <= 4.0 * np.finfo(np.float64).eps * tiny


def test_normals_stay_within_the_bound():
    assert abs(nref.Z_MAX - 5.887050112577373) < 1e-12
    # the largest radius: u(r0) smallest; the angle words at the ends and next to the axes
    ws = [0, 0xff, 0x100, 0x3fffffff, 0x40000000, 0x7fffffff, 0x80000000, 0xbfffffff, 0xc0000000, 0xffffffff]
    q = np.asarray([[0, w, 0xff, w] for w in ws], dtype=np.uint32)
    z = nref.normals_from_words(q)
    assert np.isfinite(z).all() and np.abs(z).max() <= nref.Z_MAX
    assert np.abs(np.hypot(z[:, 0], z[:, 1]) - nref.Z_MAX).max() < 1e-12
    z = nref.fill([3], None, nref.STREAM_START, 0, 1, 1 << 16)
    assert np.abs(z).max() <= nref.Z_MAX and np.abs(z.astype(np.float32)).max() <= np.float32(nref.Z_MAX)


def test_moments_of_the_reference_at_the_shared_seed():
    z = nref.fill([nref.MOMENT_SEED], None, nref.STREAM_START, 0, 1, nref.MOMENT_N)
    mean, var, kurt = nref.moments(z.astype(np.float32))
    b_mean, b_var, b_kurt = nref.moment_bounds(nref.MOMENT_N)
    print(f'[moments] mean {mean:+.3e} (<= {b_mean:.3e}), var - 1 {var - 1:+.3e} (<= {b_var:.3e}), kurtosis - 3 {kurt - 3:+.3e} (<= {b_kurt:.3e})')
    assert abs(mean) <= b_mean and abs(var - 1.0) <= b_var and abs(kurt - 3.0) <= b_kurt


def test_ulp_distance():
    a = np.asarray([1.0, -1.0, 0.0, -0.0, 1e-45], dtype=np.float32)
    b = np.asarray([np.nextafter(np.float32(1.0), np.float32(2.0)), -1.0, -0.0, 1e-45, -1e-45], dtype=np.float32)
    assert nref.ulp_distance(a, b).tolist() == [1, 0, 0, 1, 2]


# ---- 2. as_seeds -----------------------------------------------------------------------------------------------------------------
def test_as_seeds():
    assert noise.as_seeds(7, 3) == noise.Seeds((7, 8, 9))
    assert noise.as_seeds([5, 0, 2 ** 64 - 1], 3).seeds == (5, 0, 2 ** 64 - 1)
    assert noise.as_seeds((4,), 1).subs is None
    assert noise.as_seeds(np.asarray([1, 2], dtype=np.uint64), 2).seeds == (1, 2)
    assert noise.as_seeds(torch.tensor([1, 2]), 2).seeds == (1, 2)
    assert noise.as_seeds(np.int64(3), 2).seeds == (3, 4)
    sd = noise.as_seeds([1, 2, 3], 3, subs=[0, 1, 2 ** 32 - 1])
    assert sd.subs == (0, 1, 2 ** 32 - 1) and noise.as_seeds(sd, 3) is not None and noise.as_seeds(sd, 3) == sd
    assert sd.take([2, 0]) == noise.Seeds((3, 1), (2 ** 32 - 1, 0)) and len(sd) == 3
    assert noise.as_seeds([1, 2], 2, subs=5).subs == (5, 5)
    for bad, B in (([1, 2], 3), ([], 1), (-1, 1), ([-1], 1), (2 ** 64, 1), (2 ** 64 - 1, 2), ([2 ** 64], 1), (1.0, 1), ([1.5], 1), (True, 1),
                   ([True], 1), (None, 1), ('7', 1), (torch.tensor([1.0]), 1), (torch.tensor([[1]]), 1), (np.asarray([1.0]), 1), (sd, 2), (1, 0),
                   (1, -2), (1, 1.5)):
        with pytest.raises(ValueError):
            noise.as_seeds(bad, B)
    for subs in ([0], [0, -1], [0, 2 ** 32], [0, 1.5], True):
        with pytest.raises(ValueError):
            noise.as_seeds([1, 2], 2, subs=subs)
    assert (noise.STREAM_START, noise.STREAM_ETA, noise.STREAM_BLEND, noise.STREAM_POSTERIOR, noise.STREAM_USER) == (0, 1, 2, 3, 16)


def test_normal_validates_before_the_device_and_has_no_cpu_path():
    for kw in (dict(stream=-1), dict(stream=2 ** 32), dict(stream=0, row0=-1), dict(stream=0, rows=0), dict(stream=0, row0=2 ** 32 - 1, rows=2),
               dict(stream=1.0)):
        with pytest.raises(ValueError):
            noise.normal([1], (4,), device='cpu', **kw)
    for shape in ((), (0,), (4, -1)):
        with pytest.raises(ValueError):
            noise.normal([1], shape, stream=0, device='cpu')
    with pytest.raises(ValueError):
        noise.normal(7, (4,), stream=0, device='cpu')          # a start seed has no batch: as_seeds(7, B) spells it out
    with pytest.raises(mlib.MkdError, match='no CPU path'):
        noise.normal([1, 2], (4, 8, 8), stream=0, device='cpu')


# ---- 3. mkd_noise_fill's refusals ---------------------------------------------------------------------------------------------------
def test_refusals_need_no_device():
    lib = mlib.load()
    one = ctypes.c_void_p(64)          # (never dereferenced: every call below is refused on its arguments)
    ok = dict(seeds=one, subs=None, batch=2, stream=0, row0=0, rows=3, n=16, kind=0, out=one)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mkd_noise_fill(a['seeds'], a['subs'], a['batch'], a['stream'], a['row0'], a['rows'], a['n'], a['kind'], a['out'], None)
    for kw, word in ((dict(seeds=None), b'null'), (dict(out=None), b'null'), (dict(batch=0), b'>= 1'), (dict(batch=-1), b'>= 1'),
                     (dict(rows=0), b'>= 1'), (dict(rows=-3), b'>= 1'), (dict(n=0), b'>= 1'), (dict(n=-4), b'>= 1'), (dict(kind=2), b'kind'),
                     (dict(kind=-1), b'kind'), (dict(n=4 * (2 ** 32 - 1) + 1), b'32 bits'), (dict(n=2 ** 62), b'32 bits'),
                     (dict(row0=2 ** 32 - 2, rows=3), b'32 bits')):
        assert call(**kw) == -1, kw          # MKD_ERR_ARG
        assert word in lib.mkd_last_error(), (kw, lib.mkd_last_error())


# ---- 4. the seeds / x_T rules of the samplers and the model ----------------------------------------------------------------------------
def test_sampler_seed_rules_on_a_stand_in_model():
    m = HostModel(lambda x, t, c: 0.1 * x)
    x_T = torch.randn(2, 4, 3, 3)
    for smp in (DDIMSampler(m), DPMSolverSampler(m), UniPCSampler(m)):
        for bad in ([1], [1, 2, 3], -1, [1, -2], 1.5, [2 ** 64, 0]):          # validated before anything is drawn or evaluated
            with pytest.raises(ValueError):
                smp.sample(4, 2, (4, 3, 3), x_T=x_T, seeds=bad, verbose=False)
        assert not m.calls
        # seeds with x_T on a deterministic solver: x_T is taken as it is and nothing else is drawn, so a host model runs
        state = torch.get_rng_state()
        a, inter = smp.sample(4, 2, (4, 3, 3), x_T=x_T, seeds=[3, 4], eta=0.0, verbose=False)
        b, _ = smp.sample(4, 2, (4, 3, 3), x_T=x_T, eta=0.0, verbose=False)
        assert torch.equal(a, b) and inter['x_inter'][0] is x_T and torch.equal(torch.get_rng_state(), state)
        m.calls.clear()
        # without x_T the start latent is the device's: a model on the host has no device to draw on
        with pytest.raises(mlib.MkdError, match='no CPU path'):
            smp.sample(4, 2, (4, 3, 3), seeds=7, eta=0.0, verbose=False)
        assert not m.calls and torch.equal(torch.get_rng_state(), state)
    d = DDIMSampler(m)
    with pytest.raises(ValueError, match='noise_dropout'):
        d.sample(4, 2, (4, 3, 3), x_T=x_T, seeds=7, eta=1.0, noise_dropout=0.5, verbose=False)
    with pytest.raises(mlib.MkdError):          # eta > 0: the step's noise is the device's too
        d.sample(4, 2, (4, 3, 3), x_T=x_T, seeds=7, eta=1.0, verbose=False)
    d.make_schedule(4, ddim_eta=1.0, verbose=False)
    with pytest.raises(ValueError, match='repeat_noise'):
        d.p_sample_ddim(x_T, None, torch.full((2,), 1), index=1, repeat_noise=True, seeds=[1, 2], row=0)
    with pytest.raises(ValueError):
        d.stochastic_encode(x_T, [1, 1], seeds=[1])
    with pytest.raises(mlib.MkdError):
        d.stochastic_encode(x_T, [1, 1], seeds=[1, 2])
    nz = torch.randn_like(x_T)
    assert torch.equal(d.stochastic_encode(x_T, [1, 1], noise=nz, seeds=[1, 2]), d.stochastic_encode(x_T, [1, 1], noise=nz))      # noise given: taken as it is
    with pytest.raises(ValueError):          # sample_specs validates the seeds beside the specs, before the hook is called
        from makeupdiffuse_amd.batching import SampleSpec
        m.sample_rows_fast = lambda *a, **k: pytest.fail('the hook must not run')
        d.sample_specs([SampleSpec(4), SampleSpec(5)], (4, 3, 3), None, x_T=x_T, seeds=[1])
    with pytest.raises(ValueError):
        DPMSolverSampler(m).sample_specs([SampleSpec(4), SampleSpec(5)], (4, 3, 3), None, x_T=x_T, seeds=[1, 2, 3])


def test_model_seed_rules():
    small = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
                 context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
    mk = lambda **kw: TestDiffuseModel(control_stage_config={'params': dict(small, hint_channels=6, hint_widths=[16, 16, 32, 32, 32, 32, 64])},
                                       unet_config={'params': dict(small, out_channels=4)}, **kw)
    assert mk().seed is None and mk(seed=11).seed == 11 and mk(seed=2 ** 64 - 1).seed == 2 ** 64 - 1
    for bad in (-1, 2 ** 64, 1.5, '3', [1, 2], True):
        with pytest.raises(ValueError):
            mk(seed=bad)
    m = mk(seed=11)
    assert m._seeds(None, 3) == noise.Seeds((11, 12, 13)) and m._seeds([5, 6], 2) == noise.Seeds((5, 6)) and mk()._seeds(None, 3) is None
    with pytest.raises(ValueError):
        m._seeds([5], 2)
    # seeds are per source photo: the sub-stream is the face's rank
    with pytest.raises(ValueError, match='rank'):
        m.transfer_photos([torch.zeros(8, 8, 3, dtype=torch.uint8)], [torch.zeros(8, 8, 3, dtype=torch.uint8)], [(0, 0, 8, 8)], [(0, 0, 8, 8)],
                          seeds=noise.as_seeds([1], 1, subs=[0]))
    with pytest.raises(ValueError):
        m.transfer_photos([torch.zeros(8, 8, 3, dtype=torch.uint8)], [torch.zeros(8, 8, 3, dtype=torch.uint8)], [(0, 0, 8, 8)], [(0, 0, 8, 8)], seeds=[1, 2])
    # the posterior: seeds are validated, and the draw has no host path
    post = DiagonalGaussianPosterior(torch.zeros(2, 8, 2, 2))
    with pytest.raises(ValueError):
        post.sample(seeds=[1])
    with pytest.raises(mlib.MkdError):
        post.sample(seeds=[1, 2])
    state = torch.get_rng_state()
    assert post.sample().shape == (2, 4, 2, 2) and not torch.equal(torch.get_rng_state(), state)          # unseeded: the CPU generator, as before


def test_device_noise_flag_needs_a_seed():
    """--device-noise without --seed is an argument error (exit status 2, before the model is built); --seed alone keeps its meaning"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--device-noise'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--device-noise needs --seed' in r.stderr, (r.returncode, r.stderr[-400:])
    import importlib.util
    spec = importlib.util.spec_from_file_location('runs_test_cli', os.path.join(ROOT, 'runs', 'test.py'))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    a = t.build_parser().parse_args(['--seed', '3'])
    assert a.seed == 3 and a.device_noise is False
    assert t.build_parser().parse_args(['--seed', '3', '--device-noise']).device_noise is True
