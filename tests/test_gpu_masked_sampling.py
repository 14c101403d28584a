"""-m gpu: masked DDIM sampling on the device (background-preserving transfer, UPSTREAM DDIMSampler.ddim_sampling mask / x0): the
label map -> latent mask kernel and the blend kernel against their restatements, the masked in-library loop (graph replay, linear
graph segments, eager) against the per-step host loop bit for bit, mask = 0 against the unmasked loop, the step-launch count, the
small trajectory against the oracle nets inside the restated masked loop, full-size per-sample behaviour, and
TestDiffuseModel(fix_background=True).log_results."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import masked_sampling_ref as mref
import vae_encoder_ref as enc_ref
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.engine import MkdEngine, NetConfig
from oracle import nets, sampler, vae

pytestmark = pytest.mark.gpu

NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])      # f = 8
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))


def metrics(out, ref):
    out = out.float().cpu(); ref = ref.float().cpu()
    assert torch.isfinite(out).all(), 'non-finite output'
    return ((out - ref).norm() / ref.norm()).item(), F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()


@pytest.fixture(scope='module')
def mm():
    sd = nets.init_state_dict(OCFG, seed=31)
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True,
                         ddim_steps=5, unconditional_guidance_scale=9)
    m.load_state_dict({**sd, **vae.init_state_dict(vcfg, seed=32), **enc_ref.init_state_dict(vcfg, seed=33)})
    m.cuda(0)
    g = torch.Generator().manual_seed(34)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=g)
    m.save_images = False
    return m, sd


def inputs(B=2, res=64, seed=35):
    g = torch.Generator().manual_seed(seed)
    h = res // 8
    return dict(hint=torch.rand(B, 6, res, res, generator=g).to(DEV), ctx=torch.randn(B, 77, 64, generator=g).to(DEV),
                uctx=torch.randn(B, 77, 64, generator=g).to(DEV), x_T=torch.randn(B, 4, h, h, generator=g).to(DEV),
                x0=torch.randn(B, 4, h, h, generator=g).to(DEV),
                mask=(torch.rand(B, 1, h, h, generator=g) > 0.5).float().to(DEV))


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------
def test_label_mask_kernel_equals_the_reference():
    lib = L()
    g = torch.Generator().manual_seed(1)
    lab = torch.randint(0, 20, (3, 64, 48), generator=g, dtype=torch.uint8)
    lab[0, :8, :8] = 63; lab[1, :8, :8] = 200                   # label 63 in the set below; 200 never matches
    for classes in ((0, 11, 12), (1, 63), tuple(range(20))):
        bits = sum(1 << c for c in classes)
        for f in (8, 4, 16):
            for thr in (0.0, 0.5, 0.3):
                out = torch.full((3, 1, 64 // f, 48 // f), -1.0, device=DEV)
                assert lib.mkd_latent_mask_from_labels(P(lab.to(DEV)), 3, 64, 48, bits, f, thr, P(out), None) == 0
                sync()
                ref = mref.latent_mask(lab.numpy(), classes, f, thr)
                assert np.array_equal(out.cpu().numpy(), ref), f'classes {classes} f {f} threshold {thr}'
    out = torch.zeros(3, 1, 8, 8, device=DEV)
    assert lib.mkd_latent_mask_from_labels(P(lab.to(DEV)), 3, 60, 48, 1, 8, 0.5, P(out), None) == -1
    assert lib.mkd_latent_mask_from_labels(P(lab.to(DEV)), 3, 64, 48, 1, 0, 0.5, P(out), None) == -1


def test_blend_kernel_equals_the_torch_restatement():
    lib = L()
    g = torch.Generator().manual_seed(2)
    B, C, h, w = 3, 4, 9, 7
    x0, nz, x = (torch.randn(B, C, h, w, generator=g).to(DEV) for _ in range(3))
    a, b = 0.8123, 0.5832
    q = torch.full_like(x0, float('nan'))
    assert lib.mkd_q_sample_blend(P(x0), P(nz), a, b, None, 1, 1, None, P(q), B, C, h * w, None) == 0
    sync()
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    bound = 4 * 2 ** -24 * (a32 * x0.abs() + b32 * nz.abs()) + 1e-30
    assert ((q - (a32 * x0 + b32 * nz)).abs() <= bound).all(), 'q_sample'
    for mb, mc in ((B, 1), (1, C), (B, C), (1, 1)):
        mask = torch.rand(mb, mc, h, w, generator=g).to(DEV)
        out = torch.empty_like(x)
        assert lib.mkd_q_sample_blend(P(x0), P(nz), a, b, P(mask), mb, mc, P(x), P(out), B, C, h * w, None) == 0
        sync()
        ref = mref.blend(x, x0, mask, a32, b32, nz)
        bound = 4 * 2 ** -24 * ((a32 * x0.abs() + b32 * nz.abs()) * mask + (1 - mask) * x.abs()) + 1e-30
        assert ((out - ref).abs() <= bound).all(), f'mask [{mb},{mc}]'
        xi = x.clone()                                                   # in place
        assert lib.mkd_q_sample_blend(P(x0), P(nz), a, b, P(mask), mb, mc, P(xi), P(xi), B, C, h * w, None) == 0
        sync()
        assert torch.equal(xi, out)
    mask = torch.rand(2, 1, h, w, generator=g).to(DEV)
    assert lib.mkd_q_sample_blend(P(x0), P(nz), a, b, P(mask), 2, 1, P(x), P(out), B, C, h * w, None) == -1
    assert lib.mkd_q_sample_blend(P(x0), P(nz), a, b, P(mask), 1, 2, P(x), P(out), B, C, h * w, None) == -1


# ---- 2. the masked loop: every form gives the step loop's bits ------------------------------------------------------------
@pytest.mark.parametrize('eta,scale', [(0.0, 1.0), (0.0, 9.0), (0.5, 9.0), (0.5, 1.0)])
def test_masked_in_library_loop_equals_the_step_loop(mm, eta, scale):
    m, _ = mm
    I = inputs()
    c = {'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]}
    uc = {'c_crossattn': [I['uctx']], 'c_concat': [I['hint']]} if scale != 1.0 else None
    smp = DDIMSampler(m)
    S = 8                                                  # one 5-step graph + three single-step replays
    kw = dict(conditioning=c, eta=eta, x_T=I['x_T'], verbose=False, mask=I['mask'], x0=I['x0'],
              unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    outs = {}
    torch.manual_seed(40)
    outs['graph'], _ = smp.sample(S, 2, (4, 8, 8), **kw)
    m.sample_use_graph = False
    try:
        torch.manual_seed(40)
        outs['eager'], _ = smp.sample(S, 2, (4, 8, 8), **kw)
    finally:
        m.sample_use_graph = True
    torch.manual_seed(40)
    outs['steps'], _ = smp.sample(S, 2, (4, 8, 8), callback=lambda i: None, **kw)
    for k in ('eager', 'steps'):
        assert torch.equal(outs[k], outs['graph']), f'{k} != graph (eta {eta}, scale {scale})'
    torch.manual_seed(40)
    plain, _ = smp.sample(S, 2, (4, 8, 8), **{k: v for k, v in kw.items() if k not in ('mask', 'x0')})
    assert metrics(outs['graph'], plain)[0] > 1e-2                # the blend does act


def test_masked_linear_graph_segments_equal_the_eager_loop(monkeypatch):
    monkeypatch.setenv('MKD_GRAPH_MODE', '2')
    sd = nets.init_state_dict(OCFG, seed=31)
    eng = MkdEngine(NetConfig(hint_channels=6, model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2,
                              context_dim=64, hint_widths=tuple(HINT_WIDTHS)))
    eng.load_state_dict(sd)
    I = inputs()
    sch = sampler.Schedule().make_ddim(8, 0.5)
    sa, s1 = mref.sqrt_tables()
    ts = [int(t) for t in sch.ddim_timesteps]
    S = len(ts)
    g = torch.Generator().manual_seed(41)
    qk = dict(x0=I['x0'], mask=I['mask'][:1].expand(1, 4, 8, 8).contiguous(), q_sqrt_ac=[float(sa[t]) for t in ts],
              q_sqrt_1m_ac=[float(s1[t]) for t in ts], q_noise=torch.randn(S, 2, 4, 8, 8, generator=g).to(DEV))
    eta_kw = dict(sigmas=sch.ddim_sigmas, noise=torch.randn(S, 2, 4, 8, 8, generator=g).to(DEV), temperature=0.9)
    args = (ts, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
    for cfg in (1.0, 9.0):
        if cfg == 1.0:
            eng.prepare(I['hint'], I['ctx'])
        else:
            eng.prepare(torch.cat([I['hint'], I['hint']]), torch.cat([I['uctx'], I['ctx']]))
        a = eng.sample(I['x_T'], *args, cfg_scale=cfg, use_graph=False, **eta_kw, **qk)
        b = eng.sample(I['x_T'], *args, cfg_scale=cfg, use_graph=True, **eta_kw, **qk)
        u = eng.sample(I['x_T'], *args, cfg_scale=cfg, use_graph=True, **eta_kw)          # unmasked on the same cached segments
        c = eng.sample(I['x_T'], *args, cfg_scale=cfg, use_graph=True, **eta_kw, **qk)
        assert torch.equal(a, b) and torch.equal(a, c), f'segments != eager (cfg {cfg})'
        assert torch.equal(u, eng.sample(I['x_T'], *args, cfg_scale=cfg, use_graph=False, **eta_kw))
        assert metrics(a, u)[0] > 1e-2
    eng.close()


def test_zero_mask_is_the_unmasked_loop_and_launch_count_is_unchanged(mm):
    m, _ = mm
    I = inputs()
    eng = m.engine
    c = {'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]}
    uc = {'c_crossattn': [I['uctx']], 'c_concat': [I['hint']]}
    smp = DDIMSampler(m)
    for scale, ucond in ((1.0, None), (9.0, uc)):
        kw = dict(conditioning=c, eta=0.0, x_T=I['x_T'], verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=ucond)
        plain, _ = smp.sample(6, 2, (4, 8, 8), **kw)
        n_graph, n_cfg = eng.step_launches(), eng.step_launches(True, True)
        zero, _ = smp.sample(6, 2, (4, 8, 8), mask=torch.zeros(2, 1, 8, 8, device=DEV), x0=I['x0'], **kw)
        assert torch.equal(zero, plain), f'mask = 0 changed the latent (scale {scale})'
        assert eng.step_launches() == n_graph and eng.step_launches(True, True) == n_cfg
        again, _ = smp.sample(6, 2, (4, 8, 8), **kw)                   # unmasked after masked on the shared capture
        assert torch.equal(again, plain)


# ---- 3. against the oracle nets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [64, 128])
def test_masked_trajectory_vs_oracle(mm, res, monkeypatch):
    m, sd = mm
    I = inputs(res=res, seed=50 + res)
    h = res // 8
    c = {'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]}
    seen = {}
    fast = m.sample_loop_fast

    def rec(*a, **kw):
        seen.update(kw)
        return fast(*a, **kw)
    monkeypatch.setattr(m, 'sample_loop_fast', rec)
    torch.manual_seed(51)
    out, _ = DDIMSampler(m).sample(5, 2, (4, h, h), conditioning=c, x_T=I['x_T'], verbose=False, mask=I['mask'], x0=I['x0'])
    q = seen['q_noise'].cpu()
    sch = sampler.Schedule().make_ddim(5)
    ref = mref.masked_ddim(sampler.make_eps_fn(sd, OCFG), sch, I['x_T'].cpu(), {'c_crossattn': [I['ctx'].cpu()], 'c_concat': [I['hint'].cpu()]},
                           I['x0'].cpu(), I['mask'].cpu(), list(q))
    r, cs = metrics(out, ref)
    print(f'[parity] masked 5-step latent {h}x{h}: rel-L2 {r:.4e} cos {cs:.6f}')
    assert r <= 2e-2 and cs >= 0.9995


# ---- 4. full size: per-sample masks stay per-sample ------------------------------------------------------------------------
def test_full_size_batch8_masks_are_per_sample():
    eng = MkdEngine(NetConfig())
    eng.init_random(0, norm_jitter=0.2)
    g = torch.Generator().manual_seed(60)
    B, S = 8, 4
    hint = torch.rand(B, 6, 256, 256, generator=g).to(DEV)
    ctx = torch.randn(B, 77, 768, generator=g).to(DEV)
    x_T = torch.randn(B, 4, 32, 32, generator=g).to(DEV)
    x0 = torch.randn(B, 4, 32, 32, generator=g).to(DEV)
    mask = torch.stack([(torch.rand(1, 32, 32, generator=g) < (k + 1) / 9).float() for k in range(B)]).to(DEV)
    q_noise = torch.randn(S, B, 4, 32, 32, generator=g).to(DEV)
    sch = sampler.Schedule().make_ddim(S)
    sa, s1 = mref.sqrt_tables()
    ts = [int(t) for t in sch.ddim_timesteps]
    args = (ts, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
    qt = dict(q_sqrt_ac=[float(sa[t]) for t in ts], q_sqrt_1m_ac=[float(s1[t]) for t in ts])
    eng.prepare(hint, ctx)
    full = eng.sample(x_T, *args, use_graph=True, x0=x0, mask=mask, q_noise=q_noise, **qt)
    parts = []
    for lo, hi in ((0, 3), (3, 8)):
        eng.prepare(hint[lo:hi], ctx[lo:hi])
        parts.append(eng.sample(x_T[lo:hi], *args, use_graph=True, x0=x0[lo:hi], mask=mask[lo:hi],
                                q_noise=q_noise[:, lo:hi].contiguous(), **qt))
    r = metrics(torch.cat(parts), full)[0]
    print(f'[parity] full-size masked batch 8 vs 3 + 5: rel-L2 {r:.3e}')
    assert r <= 2e-2
    eng.prepare(hint, ctx)
    swapped = mask.clone(); swapped[[1, 2]] = mask[[2, 1]]
    sw = eng.sample(x_T, *args, use_graph=True, x0=x0, mask=swapped, q_noise=q_noise, **qt)
    same = [k for k in range(B) if k not in (1, 2)]
    assert torch.equal(sw[same], full[same]), 'swapping two masks changed other samples'
    for k in (1, 2):
        assert metrics(sw[k], full[k])[0] > 1e-3, f'sample {k}: its mask swap did not change it'
    eng.close()


# ---- 5. the model surface --------------------------------------------------------------------------------------------------
def test_log_results_with_fix_background(mm):
    m, _ = mm
    g = torch.Generator().manual_seed(70)
    B = 2
    seg = torch.randint(0, 15, (B, 64, 64), generator=g, dtype=torch.uint8)
    seg[:, :, :24] = 0                                      # a background band on the left
    batch = {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g),
             'txt_emb': torch.randn(B, 77, 64, generator=g), 'nonmakeup_seg': seg}
    x_T = torch.randn(B, 4, 8, 8, generator=g).to(DEV)
    base = m.log_results(batch, 0, x_T=x_T)
    assert 'mask_latent' not in base
    m.fix_background = True
    try:
        torch.manual_seed(71)
        log = m.log_results(batch, 0, x_T=x_T)
        with pytest.raises(KeyError):
            m.log_results({k: v for k, v in batch.items() if k != 'nonmakeup_seg'}, 0, x_T=x_T)
    finally:
        m.fix_background = False
    mk = log['mask_latent']
    assert tuple(mk.shape) == (B, 1, 8, 8)
    assert np.array_equal(mk.cpu().numpy(), mref.latent_mask(seg.numpy(), (0, 11, 12), 8, 0.5))
    for k in ('samples_latent', 'samples_cfg_scale_9.00_latent'):
        assert torch.isfinite(log[k]).all() and metrics(log[k], base[k])[0] > 1e-3
