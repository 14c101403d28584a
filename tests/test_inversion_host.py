"""CPU: DDIMSampler.encode (DDIM inversion, UPSTREAM DDIMSampler.encode) and DDIMSampler.decode on host stand-in models: the
update formula, the table pairing and timestep convention (decode inverts encode for an eps that ignores x), the mirrored
tables handed to the in-library loop, the eager path's triggers; and the new kernels' register budget."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import vae_encoder_ref as enc_ref
from makeupdiffuse_amd.ddim import DDIMSampler
from oracle import nets, sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostModel:
    """Stand-in model on the host: schedule tables + an eps function; no sample_loop_fast / ddim_step hooks."""

    def __init__(self, eps_fn, T=1000):
        sch = sampler.Schedule(timesteps=T)
        self.num_timesteps = T
        self.alphas_cumprod = sch.alphas_cumprod
        self.alphas_cumprod_prev = sch.alphas_cumprod_prev
        self.betas = torch.tensor(np.diff(np.append(0.0, 1.0 - sch.alphas_cumprod64)), dtype=torch.float32)
        self.sqrt_one_minus_alphas_cumprod = sch.sqrt_one_minus_alphas_cumprod
        self.device = torch.device('cpu')
        self.eps_fn = eps_fn
        self.calls = []

    def apply_model(self, x, t, c):
        self.calls.append(t.clone())
        return self.eps_fn(x, t, c)


def upstream_encode(model, s, x0, c, t_enc, scale=1.0, uc=None):
    """the upstream loop, written out (with the model evaluated at ddim_timesteps[i])"""
    x = x0
    for i in range(t_enc):
        a_next = float(s.ddim_alphas[i]); a = float(s.ddim_alphas_prev[i])
        t = torch.full((x.shape[0],), int(s.ddim_timesteps[i]), dtype=torch.long)
        if uc is None or scale == 1.0:
            e = model.eps_fn(x, t, c)
        else:
            cc = {'c_crossattn': [torch.cat([uc['c_crossattn'][0], c['c_crossattn'][0]])], 'c_concat': None}
            e_u, e_c = model.eps_fn(torch.cat([x, x]), torch.cat([t, t]), cc).chunk(2)
            e = e_u + scale * (e_c - e_u)
        x = (a_next / a) ** 0.5 * x + a_next ** 0.5 * ((1 / a_next - 1) ** 0.5 - (1 / a - 1) ** 0.5) * e
    return x


SMALL = nets.NetConfig(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=32,
                       hint_widths=(16, 16, 32, 32, 32, 32, 32))


def test_encode_on_an_oracle_model_matches_the_upstream_formula():
    sd = nets.init_state_dict(SMALL, seed=1)
    m = HostModel(sampler.make_eps_fn(sd, SMALL))
    s = DDIMSampler(m)
    s.make_schedule(ddim_num_steps=10, verbose=False)
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, 4, 4, 4, generator=g)
    c = {'c_crossattn': [torch.randn(2, 77, 32, generator=g)], 'c_concat': None}
    uc = {'c_crossattn': [torch.randn(2, 77, 32, generator=g)], 'c_concat': None}
    out, info = s.encode(x0, c, 4)
    torch.testing.assert_close(out, upstream_encode(m, s, x0, c, 4), rtol=1e-5, atol=1e-5)
    assert info['x_encoded'] is out and info['intermediate_steps'] == [] and 'intermediates' not in info
    ref = enc_ref.ddim_invert(m.eps_fn, s.ddim_timesteps, s.ddim_alphas, s.ddim_alphas_prev, x0, c, 4)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    outc, _ = s.encode(x0, c, 3, unconditional_guidance_scale=4.0, unconditional_conditioning=uc)
    torch.testing.assert_close(outc, upstream_encode(m, s, x0, c, 3, 4.0, uc), rtol=1e-5, atol=1e-5)


def test_decode_inverts_encode_for_an_eps_that_ignores_x():
    g = torch.Generator().manual_seed(3)
    e_fix = torch.randn(2, 4, 8, 8, generator=g)
    m = HostModel(lambda x, t, c: e_fix * (1.0 + t.float().view(-1, 1, 1, 1) / 1000.0))      # depends on t, not on x
    s = DDIMSampler(m)
    s.make_schedule(ddim_num_steps=20, verbose=False)
    x0 = torch.randn(2, 4, 8, 8, generator=g)
    for n in (1, 7, 20):
        xe, _ = s.encode(x0, {}, n)
        back = s.decode(xe, {}, n)
        torch.testing.assert_close(back, x0, rtol=1e-5, atol=1e-5)
    m.calls.clear()
    s.encode(x0, {}, 3)
    assert [int(t[0]) for t in m.calls] == [int(v) for v in s.ddim_timesteps[:3]]


def test_in_library_loop_gets_the_mirrored_tables():
    m = HostModel(lambda x, t, c: torch.zeros_like(x))
    seen = {}

    def fast(x, c, timesteps, alphas, alphas_prev, s1m, scale=1.0, uc=None):
        seen.update(timesteps=list(timesteps), alphas=list(alphas), alphas_prev=list(alphas_prev), s1m=list(s1m), scale=scale, uc=uc)
        return x + 1

    m.sample_loop_fast = fast
    s = DDIMSampler(m)
    s.make_schedule(ddim_num_steps=10, verbose=False)
    x0 = torch.zeros(1, 4, 2, 2)
    out, info = s.encode(x0, {'c': 1}, 6, unconditional_guidance_scale=3.0, unconditional_conditioning={'u': 1})
    assert torch.equal(out, x0 + 1) and info['x_encoded'] is out
    n = 6
    for j in range(n):
        k = n - 1 - j
        assert seen['timesteps'][j] == int(s.ddim_timesteps[k])
        assert seen['alphas'][j] == float(s.ddim_alphas_prev[k])
        assert seen['alphas_prev'][j] == float(s.ddim_alphas[k])
        assert abs(seen['s1m'][j] - float(np.sqrt(1.0 - np.float32(s.ddim_alphas_prev[k])))) < 1e-7
    assert seen['scale'] == 3.0 and seen['uc'] == {'u': 1}
    # eager path: callback, return_intermediates, use_original_steps
    seen.clear()
    got = []
    s.encode(x0, {}, 4, callback=got.append)
    assert got == [0, 1, 2, 3] and not seen
    _, info = s.encode(x0, {}, 6, return_intermediates=2)
    assert not seen and info['intermediate_steps'] == [0, 3, 4, 5] and len(info['intermediates']) == 4
    s.encode(x0, {}, 3, use_original_steps=True)
    assert not seen
    with pytest.raises(ValueError):
        s.encode(x0, {}, 11)


def test_new_kernels_compile_without_scratch_or_spills(tmp_path):
    """the encoder's kernels (3-channel conv_in, fused tail) for gfx950: no private segment, no VGPR / SGPR spills."""
    src = os.path.join(ROOT, 'makeupdiffuse_amd', 'csrc', 'kernels_misc.hip')
    hipcc = next((p for p in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc') if p and os.path.exists(p)), None)
    if hipcc is None:
        pytest.fail('hipcc not found')
    asm = tmp_path / 'misc.s'
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=fast', '--cuda-device-only', '-S',
                           src, '-o', str(asm)])
    text = asm.read_text()
    found = 0
    for name in ('vae_enc_tail_kernel', 'conv3x3_fewin_kernelILi3E'):
        blocks = [m for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.S) if name in m.group(1)]
        assert blocks, f'{name} not in the device code'
        for b in blocks:
            assert re.search(r'\.amdhsa_private_segment_fixed_size 0\n', b.group(2)), f'{b.group(1)} uses scratch'
            found += 1
    for m in re.finditer(r'\.name:\s+(\S+)\n(?:.*\n){0,40}?\s+\.vgpr_spill_count:\s+(\d+)', text):
        if 'vae_enc_tail' in m.group(1) or 'fewin_kernelILi3E' in m.group(1):
            assert int(m.group(2)) == 0, f'{m.group(1)} spills VGPRs'
    assert found >= 2
