"""CPU: masked DDIM sampling (background-preserving transfer, UPSTREAM DDIMSampler.ddim_sampling mask / x0) on host stand-in
models: the blend against the upstream loop written out, the draw order handed to the in-library loop, argument errors, the
label map -> latent mask reference, DDIMSampler.stochastic_encode, the seg-carrying dataset, and the new kernels' register budget."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import masked_sampling_ref as mref
from makeupdiffuse_amd.ddim import DDIMSampler
from oracle import nets, sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostModel:
    """Stand-in model on the host: schedule tables (incl. the q_sample pair) + an eps function; no device hooks."""

    def __init__(self, eps_fn, T=1000):
        sch = sampler.Schedule(timesteps=T)
        self.num_timesteps = T
        self.alphas_cumprod = sch.alphas_cumprod
        self.alphas_cumprod_prev = sch.alphas_cumprod_prev
        self.betas = torch.tensor(np.diff(np.append(0.0, 1.0 - sch.alphas_cumprod64)), dtype=torch.float32)
        self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod = mref.sqrt_tables(T)
        self.device = torch.device('cpu')
        self.eps_fn = eps_fn

    def apply_model(self, x, t, c):
        return self.eps_fn(x, t, c)


SMALL = nets.NetConfig(model_channels=32, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=32,
                       hint_widths=(16, 16, 32, 32, 32, 32, 32))


@pytest.fixture(scope='module')
def oracle_model():
    sd = nets.init_state_dict(SMALL, seed=4)
    return HostModel(sampler.make_eps_fn(sd, SMALL))


@pytest.mark.parametrize('eta', [0.0, 0.6])
@pytest.mark.parametrize('cfg', [False, True])
@pytest.mark.parametrize('per_sample', [True, False])
def test_masked_sample_on_an_oracle_model_matches_the_upstream_loop(oracle_model, eta, cfg, per_sample):
    m = oracle_model
    S, B = 4, 2
    g = torch.Generator().manual_seed(11)
    x_T = torch.randn(B, 4, 4, 4, generator=g)
    x0 = torch.randn(B, 4, 4, 4, generator=g)
    mask = (torch.rand((B, 1, 4, 4) if per_sample else (1, 4, 4, 4), generator=g) > 0.5).float()
    mask[..., 0, 0] = 0.25                               # a soft entry too
    c = {'c_crossattn': [torch.randn(B, 77, 32, generator=g)], 'c_concat': None}
    uc = {'c_crossattn': [torch.randn(B, 77, 32, generator=g)], 'c_concat': None} if cfg else None
    scale = 5.0 if cfg else 1.0
    s = DDIMSampler(m)
    torch.manual_seed(123)
    out, _ = s.sample(S, B, (4, 4, 4), conditioning=c, eta=eta, x_T=x_T, verbose=False, mask=mask, x0=x0,
                      unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    # the same draws in the upstream order: each step's q_sample noise (randn_like(x0)), then its eta noise (sigma_t != 0 only)
    sch = sampler.Schedule().make_ddim(S, eta)
    torch.manual_seed(123)
    q_draws, eta_draws = [], []
    for i in range(S):
        q_draws.append(torch.randn_like(x0))
        eta_draws.append(torch.randn(x_T.shape) if float(sch.ddim_sigmas[S - 1 - i]) != 0.0 else None)
    ref = mref.masked_ddim(m.eps_fn, sch, x_T, c, x0, mask, q_draws, eta_draws, scale, uc)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    # the blend does act (not a vacuous comparison): the unmasked loop differs, and mask = 1 everywhere keeps the x0 side
    plain, _ = s.sample(S, B, (4, 4, 4), conditioning=c, eta=0.0, x_T=x_T, verbose=False,
                        unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    assert (out - plain).abs().max() > 1e-3


def test_fast_path_gets_the_draws_of_the_step_loop_in_its_order(monkeypatch):
    """The in-library loop is handed [steps, ...] rows equal to what the step loop draws under the same seed: per step the
    blend's randn_like(x0) first, then the eta draw; plus the DDPM tables at each entry's timestep."""
    m = HostModel(lambda x, t, c: 0.1 * x)
    S, B = 5, 2
    x_T = torch.randn(B, 4, 3, 3)
    x0 = torch.randn(B, 4, 3, 3)
    mask = torch.ones(B, 1, 3, 3)
    seen = {}

    def fast(x, c, timesteps, alphas, alphas_prev, s1m, scale=1.0, uc=None, **kw):
        seen.update(kw, timesteps=list(timesteps))
        return x

    for eta in (0.0, 0.5):
        m.sample_loop_fast = fast
        seen.clear()
        torch.manual_seed(9)
        DDIMSampler(m).sample(S, B, (4, 3, 3), conditioning={}, eta=eta, x_T=x_T, verbose=False, mask=mask, x0=x0)
        assert seen['x0'] is x0 and seen['mask'] is mask
        assert tuple(seen['q_noise'].shape) == (S, B, 4, 3, 3)
        ts = seen['timesteps']
        assert seen['q_sqrt_ac'] == [float(m.sqrt_alphas_cumprod[t]) for t in ts]
        assert seen['q_sqrt_1m_ac'] == [float(m.sqrt_one_minus_alphas_cumprod[t]) for t in ts]
        assert ('noise' in seen) == (eta > 0)
        # the step loop under the same seed, recording every draw in order
        del m.sample_loop_fast
        drawn = []
        real_like, real_randn = torch.randn_like, torch.randn

        def rec_like(t, *a, **k):
            v = real_like(t, *a, **k); drawn.append(('q', v)); return v

        def rec_randn(*a, **k):
            v = real_randn(*a, **k); drawn.append(('eta', v)); return v
        monkeypatch.setattr(torch, 'randn_like', rec_like)
        monkeypatch.setattr(torch, 'randn', rec_randn)
        torch.manual_seed(9)
        DDIMSampler(m).sample(S, B, (4, 3, 3), conditioning={}, eta=eta, x_T=x_T, verbose=False, mask=mask, x0=x0)
        monkeypatch.undo()
        kinds = [k for k, _ in drawn]
        assert kinds == (['q', 'eta'] * S if eta > 0 else ['q'] * S)
        q_rows = [v for k, v in drawn if k == 'q']
        assert torch.equal(seen['q_noise'], torch.stack(q_rows))
        if eta > 0:
            assert torch.equal(seen['noise'], torch.stack([v for k, v in drawn if k == 'eta']))


def test_fast_path_draw_count_with_a_zero_sigma_and_dropout():
    """The generator's use on the unseeded masked eta fast path, replayed by hand: x_T first, then for each executed step the blend's
    randn_like(x0) and the step's eta draw with the dropout applied to it; a step whose sigma is 0 gets zeros and no draw; nothing is
    drawn after the last step (the generator ends in the replay's state)."""
    m = HostModel(lambda x, t, c: 0.1 * x)
    shape = (2, 4, 3, 3)
    x0 = torch.randn(shape)
    mask = torch.ones(2, 1, 3, 3)
    seen = {}

    def fast(x, c, timesteps, alphas, alphas_prev, s1m, scale=1.0, uc=None, **kw):
        seen.update(kw, x=x)
        return x

    m.sample_loop_fast = fast
    smp = DDIMSampler(m)
    smp.make_schedule(5, ddim_eta=0.5, verbose=False)
    smp.ddim_sigmas[1] = 0.0
    n = len(smp.ddim_timesteps)
    torch.manual_seed(21)
    smp.ddim_sampling({}, shape, mask=mask, x0=x0, noise_dropout=0.25)
    state = torch.get_rng_state()
    torch.manual_seed(21)
    x_T = torch.randn(shape)
    q_rows, eta_rows = [], []
    for k in range(n):
        q_rows.append(torch.randn_like(x0))
        if float(smp.ddim_sigmas[n - 1 - k]) != 0.0:
            eta_rows.append(torch.nn.functional.dropout(torch.randn(shape), p=0.25))
        else:
            eta_rows.append(torch.zeros(shape))
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(seen['x'], x_T)
    assert torch.equal(seen['q_noise'], torch.stack(q_rows))
    assert torch.equal(seen['noise'], torch.stack(eta_rows)) and not seen['noise'][n - 2].any() and seen['noise'][0].any()


def test_mask_errors():
    m = HostModel(lambda x, t, c: torch.zeros_like(x))
    s = DDIMSampler(m)
    x_T = torch.zeros(2, 4, 4, 4)
    x0 = torch.zeros(2, 4, 4, 4)
    with pytest.raises(ValueError):
        s.sample(2, 2, (4, 4, 4), conditioning={}, x_T=x_T, verbose=False, mask=torch.ones(2, 1, 4, 4))      # mask without x0
    for bad in (torch.ones(3, 1, 4, 4), torch.ones(2, 2, 4, 4), torch.ones(2, 1, 4, 5), torch.ones(2, 4, 4), torch.ones(1, 1, 8, 8)):
        with pytest.raises(ValueError):
            s.sample(2, 2, (4, 4, 4), conditioning={}, x_T=x_T, verbose=False, mask=bad, x0=x0)
    with pytest.raises(ValueError):
        s.sample(2, 2, (4, 4, 4), conditioning={}, x_T=x_T, verbose=False, mask=torch.ones(2, 1, 4, 4), x0=torch.zeros(4, 4, 4, 4))
    for k in ('score_corrector', 'dynamic_threshold', 'ucg_schedule', 'corrector_kwargs'):
        with pytest.raises(NotImplementedError):
            s.sample(2, 2, (4, 4, 4), conditioning={}, x_T=x_T, verbose=False, **{k: object()})
    for ok in (torch.ones(1, 1, 4, 4), torch.ones(2, 4, 4, 4), torch.ones(1, 4, 4, 4)):
        s.sample(2, 2, (4, 4, 4), conditioning={}, x_T=x_T, verbose=False, mask=ok, x0=x0)


NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])


def _model(**kw):
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    return TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=[16, 16, 32, 32, 32, 32, 64])},
                            unet_config={'params': dict(NET, out_channels=4)},
                            first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, **kw)


def test_fix_background_settings_and_errors():
    m = _model()
    assert m.fix_background is False and m.background_classes == (0, 11, 12) and m.background_threshold == 0.5
    assert m.seg_key == 'nonmakeup_seg'
    m2 = _model(fix_background=True, background_classes=[0, 12], background_threshold=0.0, seg_key='seg')
    assert m2.fix_background and m2.background_classes == (0, 12) and m2.background_threshold == 0.0 and m2.seg_key == 'seg'
    batch = {'src_img': torch.rand(1, 3, 64, 64), 'ref_img': torch.rand(1, 3, 64, 64), 'txt_emb': torch.zeros(1, 77, 64)}
    with pytest.raises(ValueError, match='first_stage_encoder'):
        _model(fix_background=True).log_results(batch, 0)
    with pytest.raises(KeyError, match='nonmakeup_seg'):
        _model(fix_background=True, first_stage_encoder=True).log_results(batch, 0)


def test_latent_mask_reference_on_hand_made_label_maps():
    f = 8
    lab = np.full((2, 16, 24), 1, dtype=np.uint8)            # skin everywhere
    lab[0, :8, :8] = 0                                       # block (0,0): all background
    lab[0, :8, 8:16] = 11                                    # block (0,1): top half teeth, bottom half hair -> all kept
    lab[0, 4:8, 8:16] = 12
    lab[0, 8:16, 0:8] = 1                                    # block (1,0): 16 background + 16 teeth + 32 skin -> 0.5
    lab[0, 8:10, 0:8] = 0
    lab[0, 10:12, 0:8] = 11
    lab[0, 8:16, 8:16] = 10                                  # block (1,1): neck (not in the set) 33, background 31 -> 31/64
    lab[0, 8:16, 8:12] = 0
    lab[0, 8, 8] = 10
    lab[1, :, 16:] = 12                                      # sample 1: the right third is hair
    soft = mref.latent_mask(lab, (0, 11, 12), f, 0.0)
    assert soft.shape == (2, 1, 2, 3) and soft.dtype == np.float32
    np.testing.assert_array_equal(soft[0, 0], np.array([[1.0, 1.0, 0.0], [0.5, 31 / 64, 0.0]], np.float32))
    np.testing.assert_array_equal(soft[1, 0], np.array([[0, 0, 1], [0, 0, 1]], np.float32))
    hard = mref.latent_mask(lab, (0, 11, 12), f, 0.5)
    np.testing.assert_array_equal(hard[0, 0], np.array([[1, 1, 0], [1, 0, 0]], np.float32))
    # the soft mask is the area average of the binary mask
    binary = torch.from_numpy(np.isin(lab, [0, 11, 12]).astype(np.float32))[:, None]
    np.testing.assert_array_equal(F.interpolate(binary, scale_factor=1 / f, mode='area').numpy(), soft)
    # other class sets / factors
    only_bg = mref.latent_mask(lab, (0,), 4, 0.0)
    assert only_bg.shape == (2, 1, 4, 6) and float(only_bg[0, 0, 0, 0]) == 1.0 and float(only_bg[0, 0, 1, 2]) == 0.0


def test_stochastic_encode_equals_its_formula():
    m = HostModel(lambda x, t, c: torch.zeros_like(x))
    s = DDIMSampler(m)
    s.make_schedule(ddim_num_steps=10, verbose=False)
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(3, 4, 5, 5, generator=g)
    noise = torch.randn(3, 4, 5, 5, generator=g)
    for t in (torch.tensor([4, 4, 4]), torch.tensor([0, 7, 9])):
        want = torch.sqrt(s.ddim_alphas)[t].view(-1, 1, 1, 1) * x0 + s.ddim_sqrt_one_minus_alphas[t].view(-1, 1, 1, 1) * noise
        torch.testing.assert_close(s.stochastic_encode(x0, t, noise=noise), want, rtol=0, atol=0)
    t = torch.tensor([10, 500, 999])
    want = s.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1) * x0 + s.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1) * noise
    torch.testing.assert_close(s.stochastic_encode(x0, t, use_original_steps=True, noise=noise), want, rtol=0, atol=0)
    torch.manual_seed(3)
    a = s.stochastic_encode(x0, torch.tensor([2, 2, 2]))
    torch.manual_seed(3)
    n = torch.randn_like(x0)
    torch.testing.assert_close(a, float(torch.sqrt(s.ddim_alphas)[2]) * x0 + float(s.ddim_sqrt_one_minus_alphas[2]) * n)
    with pytest.raises(ValueError):
        s.stochastic_encode(x0, torch.tensor([1, 2]), noise=noise)


def test_pair_folder_dataset_loads_label_maps(tmp_path):
    from PIL import Image
    from makeupdiffuse_amd import imageio as mio
    for d in ('images', 'scgan_segs'):
        (tmp_path / d).mkdir()
    rng = np.random.default_rng(1)
    Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / 'images' / 'a.png')
    Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / 'images' / 'b.png')
    sa = rng.integers(0, 15, (32, 32), dtype=np.uint8)
    sb = np.zeros((64, 64), np.uint8); sb[:, 32:] = 12
    Image.fromarray(sa).save(tmp_path / 'scgan_segs' / 'a.png'); Image.fromarray(sb).save(tmp_path / 'scgan_segs' / 'b.png')
    (tmp_path / 'pairs.txt').write_text('a.png b.png\n')
    it = mio.PairFolderDataset(str(tmp_path), 'pairs.txt', dim=(32, 32))[0]
    assert it['nonmakeup_seg'].dtype == torch.uint8 and tuple(it['nonmakeup_seg'].shape) == (32, 32)
    assert np.array_equal(it['nonmakeup_seg'].numpy(), sa)
    mk = it['makeup_seg'].numpy()                             # resized with nearest: still only the labels 0 and 12
    assert mk.shape == (32, 32) and set(np.unique(mk)) == {0, 12} and (mk[:, 16:] == 12).all() and (mk[:, :16] == 0).all()
    batch = mio.collate([it, it])
    assert tuple(batch['nonmakeup_seg'].shape) == (2, 32, 32)
    (tmp_path / 'scgan_segs' / 'a.png').unlink(); (tmp_path / 'scgan_segs' / 'b.png').unlink(); (tmp_path / 'scgan_segs').rmdir()
    assert 'nonmakeup_seg' not in mio.PairFolderDataset(str(tmp_path), 'pairs.txt', dim=(32, 32))[0]


def test_masked_sampling_kernels_compile_without_scratch_or_spills(tmp_path):
    """the step setup (now with the blend), the stand-alone blend and the label -> mask kernel for gfx950: no private segment, no
    VGPR spills"""
    src = os.path.join(ROOT, 'makeupdiffuse_amd', 'csrc', 'kernels_misc.hip')
    hipcc = next((p for p in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc') if p and os.path.exists(p)), None)
    if hipcc is None:
        pytest.fail('hipcc not found')
    asm = tmp_path / 'misc.s'
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=fast', '--cuda-device-only', '-S',
                           src, '-o', str(asm)])
    text = asm.read_text()
    names = ('step_setup_kernel', 'q_sample_blend_kernel', 'latent_mask_from_labels_kernel')
    for name in names:
        blocks = [mm for mm in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.S) if name in mm.group(1)]
        assert blocks, f'{name} not in the device code'
        for b in blocks:
            assert re.search(r'\.amdhsa_private_segment_fixed_size 0\n', b.group(2)), f'{b.group(1)} uses scratch'
    for mm in re.finditer(r'\.name:\s+(\S+)\n(?:.*\n){0,40}?\s+\.vgpr_spill_count:\s+(\d+)', text):
        if any(n in mm.group(1) for n in names):
            assert int(mm.group(2)) == 0, f'{mm.group(1)} spills VGPRs'
