"""-m gpu: the first-stage ENCODER (get_z = get_first_stage_encoding(encode_first_stage(x))) and the DDIM inversion on the
device: the Downsample on the gather kernel (bottom/right-only pad, stride 2), the 3-channel conv_in, the fused encoder tail,
the encoder plan against the fp32 restatement (tests/vae_encoder_ref.py), its workspace being its own, and
DDIMSampler.encode through the in-library loop."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, L, P, assert_close_bf16, bf, sync
import vae_encoder_ref as enc_ref
from makeupdiffuse_amd.engine import MkdEngine, NetConfig, VaeConfig
from makeupdiffuse_amd.lib import MkdError
from oracle import nets, sampler, vae

pytestmark = pytest.mark.gpu

SMALL = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
             hint_widths=(16, 16, 32, 32, 32, 32, 64))
GATHER_CFGS = [0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36,
               37, 41, 44, 45, 46, 47, 48, 49, 50]


def metrics(out, ref):
    out = out.float().cpu(); ref = ref.float().cpu()
    assert torch.isfinite(out).all(), 'non-finite output'
    return ((out - ref).norm() / ref.norm()).item(), F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()


def check(out, ref, rel, cos, what):
    r, c = metrics(out, ref)
    print(f'[parity] {what}: rel-L2 {r:.4e} cos {c:.6f} (limits {rel:g} / {cos:g})')
    assert r <= rel and c >= cos, f'{what}: rel-L2 {r:.4e} (<= {rel}), cos {c:.6f} (>= {cos})'
    return r, c


def packed(w):
    Cout, Cin = w.shape[:2]
    wp = torch.empty(Cout, 9 * Cin, device=DEV, dtype=torch.bfloat16)
    assert L().mkd_pack_conv_weight(P(w.float().contiguous()), P(wp), Cout, Cin, 3, 3, None) == 0
    return wp


# ---- 1. Downsample on the gather kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', GATHER_CFGS)
@pytest.mark.parametrize('splitk', [1, 0])
@pytest.mark.parametrize('B,H,W_,Cin,Cout', [(1, 16, 24, 64, 128), (3, 10, 14, 320, 256), (3, 16, 24, 128, 64), (1, 64, 64, 256, 320)])
def test_downsample_conv_every_gather_tile(cfg, splitk, B, H, W_, Cin, Cout):
    lib = L()
    g = torch.Generator().manual_seed(cfg * 31 + B * H + Cin + Cout)
    xb = bf(torch.randn(B, Cin, H, W_, generator=g))
    wbf = bf(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    bias = torch.randn(Cout, generator=g).to(DEV)
    xn = xb.permute(0, 2, 3, 1).contiguous()
    wp = packed(wbf)
    y = torch.zeros(B, H // 2, W_ // 2, Cout, device=DEV, dtype=torch.bfloat16)
    lib.mkd_gemm_force_tile(cfg)
    try:
        rc = lib.mkd_conv3x3_down_bf16(P(xn), Cin, P(wp), P(bias), P(y), Cout, B, H, W_, Cin, Cout, splitk, None)
        assert rc == 0, lib.mkd_last_error()
        sync()
    finally:
        lib.mkd_gemm_force_tile(-1)
    ref = F.conv2d(F.pad(xb.float(), (0, 1, 0, 1)), wbf.float(), bias, stride=2)
    assert ref.shape[2:] == (H // 2, W_ // 2)
    assert_close_bf16(y.float().permute(0, 3, 1, 2), ref, what=f'downsample cfg {cfg} splitk {splitk}')


def test_downsample_conv_refuses_odd_sizes():
    lib = L()
    x = torch.zeros(1, 9, 8, 64, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(64, 9 * 64, device=DEV, dtype=torch.bfloat16)
    y = torch.zeros(1, 5, 4, 64, device=DEV, dtype=torch.bfloat16)
    assert lib.mkd_conv3x3_down_bf16(P(x), 64, P(w), None, P(y), 64, 1, 9, 8, 64, 64, 0, None) == -1


# ---- 2. 3-channel conv_in ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cout', [64, 128, 320, 32])
def test_conv_in_three_channels(Cout):
    lib = L()
    g = torch.Generator().manual_seed(Cout)
    B, H, W_ = 2, 40, 24
    x = torch.randn(B, 3, H, W_, generator=g).to(DEV)
    w = bf(torch.randn(Cout, 3, 3, 3, generator=g) / math.sqrt(27))
    bias = torch.randn(Cout, generator=g).to(DEV)
    wp = torch.empty(Cout, 27, device=DEV, dtype=torch.bfloat16)
    assert lib.mkd_pack_conv_weight(P(w.float().contiguous()), P(wp), Cout, 3, 3, 3, None) == 0
    out = torch.zeros(B, H, W_, Cout, device=DEV, dtype=torch.bfloat16)
    rc = lib.mkd_conv3x3_direct(P(x), 1, P(wp), P(bias), P(out), 0, 0, None, B, H, W_, 3, Cout, 1, None)
    assert rc == 0, lib.mkd_last_error()
    sync()
    assert_close_bf16(out.float().permute(0, 3, 1, 2), F.conv2d(x, w.float(), bias, padding=1), what=f'conv_in 3->{Cout}')


# ---- 3./4. the encoder against the restatement -----------------------------------------------------------------------
def make_encoder(ocfg, seed, with_decoder=False):
    sd = enc_ref.init_state_dict(ocfg, seed=seed)
    eng = MkdEngine(NetConfig(**SMALL))
    vc = VaeConfig(z_channels=ocfg.z_channels, embed_dim=ocfg.embed_dim, ch=ocfg.ch, ch_mult=tuple(ocfg.ch_mult),
                   num_res_blocks=ocfg.num_res_blocks, out_ch=ocfg.out_ch)
    dsd = None
    if with_decoder:
        eng.configure_vae(vc)
        dsd = vae.init_state_dict(ocfg, seed=seed + 1)
        for k, v in dsd.items():
            eng.load_weight(k, v)
        eng.finalize_vae()
    eng.configure_vae_encoder(vc)
    for k, v in sd.items():
        eng.load_weight(k, v)
    eng.finalize_vae_encoder()
    return eng, sd, dsd


@pytest.mark.parametrize('ch_mult', [(1, 2), (1, 2, 2)])
def test_encoder_small_vs_restatement(ch_mult):
    ocfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=ch_mult, num_res_blocks=1, out_ch=3)
    eng, sd, _ = make_encoder(ocfg, seed=11)
    exp = {k for k in eng.expected_params() if k.startswith('first_stage_model.')}
    assert exp == set(enc_ref.param_spec(ocfg)), exp ^ set(enc_ref.param_spec(ocfg))
    f = 2 ** (len(ch_mult) - 1)
    gen = torch.Generator().manual_seed(4)
    for B, H, W_ in [(2, 64, 96), (3, 48, 80)]:
        x = torch.rand(B, 3, H, W_, generator=gen) * 2 - 1
        noise = torch.randn(B, 4, H // f, W_ // f, generator=gen)
        mom_ref = enc_ref.moments(sd, ocfg, x)
        z, mom = eng.encode(x, 0.18215, None, moments=True)
        assert mom.shape == mom_ref.shape == (B, 8, H // f, W_ // f)
        check(mom, mom_ref, 1.5e-2, 0.9997, f'moments {ch_mult} {B}x{H}x{W_}')
        check(z, enc_ref.latent(mom_ref, None), 1.5e-2, 0.9997, f'mode() latent {ch_mult} {B}x{H}x{W_}')
        zs = eng.encode(x, 0.18215, noise)
        check(zs, enc_ref.latent(mom_ref, noise), 1.5e-2, 0.9997, f'sampled latent {ch_mult} {B}x{H}x{W_}')
        # the tail computes sample() from ITS moments: exact up to fp32 rounding of exp
        torch.testing.assert_close(zs.cpu(), enc_ref.latent(mom.cpu(), noise), rtol=1e-5, atol=1e-5)
    eng.close()


@pytest.mark.timeout(1200)
def test_encoder_full_size():
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    eng, sd, _ = make_encoder(vae.FULL, seed=0)
    spec = enc_ref.param_spec(vae.FULL)
    exp = {k: v for k, v in eng.expected_params().items() if k.startswith('first_stage_model.')}
    assert exp == spec
    assert eng.param_count('vae_encoder') == 34163664
    gen = torch.Generator().manual_seed(7)
    for B, H in [(2, 256), (1, 512)]:
        x = torch.rand(B, 3, H, H, generator=gen) * 2 - 1
        _, mom = eng.encode(x, 0.18215, None, moments=True)
        r, c = check(mom, enc_ref.moments(sd, vae.FULL, x), 2e-2, 0.9995, f'full encoder {B}x{H}^2')
    print(f'full encoder GFLOP at 1x512^2: {eng.encode_flops() / 1e9:.1f}')
    x8 = torch.rand(8, 3, 256, 256, generator=gen) * 2 - 1
    z8 = eng.encode(x8).cpu()
    z35 = torch.cat([eng.encode(x8[:3]).cpu(), eng.encode(x8[3:]).cpu()])
    check(z8, z35, 2e-2, 0.9999, 'B=8 == B=3 + B=5')
    eng.close()


# ---- 5. workspace independence ----------------------------------------------------------------------------------------
def test_encoder_workspace_does_not_move_the_decoder():
    ocfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, out_ch=3)
    eng, _, _ = make_encoder(ocfg, seed=3, with_decoder=True)
    z = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(1)) * 0.18215
    d1 = eng.decode(z).cpu()
    eng.encode(torch.rand(8, 3, 512, 512, generator=torch.Generator().manual_seed(2)) * 2 - 1)
    d2 = eng.decode(z).cpu()
    assert torch.equal(d1, d2)
    eng.close()
    dec_only = MkdEngine(NetConfig(**SMALL))
    dec_only.configure_vae(VaeConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1))
    keys = [k for k in dec_only.expected_params() if k.startswith(MkdEngine.VAE_ENCODER_PREFIXES)]
    assert keys == [] and dec_only.param_count('vae_encoder') == 0
    dec_only.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------
def test_encode_errors():
    lib = L()
    eng, _, _ = make_encoder(vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3), seed=2)
    x = torch.zeros(1, 3, 100, 104, device=DEV)
    z = torch.zeros(1, 4, 16, 16, device=DEV)
    for H, W_ in [(100, 104), (36, 40)]:
        assert lib.mkd_encode(eng._ctx, P(x), 1, H, W_, 0.18215, None, P(z), None, None) == -1
    assert lib.mkd_encode(eng._ctx, P(x), 1, 64, 64, 0.18215, None, None, None, None) == -1
    eng.close()
    plain = MkdEngine(NetConfig(**SMALL))
    assert lib.mkd_encode(plain._ctx, P(x), 1, 64, 64, 0.18215, None, P(z), None, None) == -3
    with pytest.raises(MkdError):
        plain.encode(torch.zeros(1, 3, 64, 64))
    plain.close()


# ---- 7./8. inversion and the class surface ------------------------------------------------------------------------------
NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])      # f = 8: latent = hint / 8


@pytest.fixture(scope='module')
def inv_model():
    from makeupdiffuse_amd.diffmk.makeups import BaseModel
    ocfg = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                          hint_widths=tuple(HINT_WIDTHS), hint_channels=3)
    sd = nets.init_state_dict(ocfg, seed=21)
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    vsd = vae.init_state_dict(vcfg, seed=22)
    esd = enc_ref.init_state_dict(vcfg, seed=23)
    m = BaseModel(control_stage_config={'params': dict(NET, hint_channels=3, hint_widths=HINT_WIDTHS)},
                  unet_config={'params': dict(NET, out_channels=4)},
                  first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True,
                  iter_finetune=5)
    m.load_state_dict({**sd, **vsd, **esd})
    m.cuda(0)
    return m, ocfg, sd, vcfg, vsd, esd


def test_inversion_in_library_loop_equals_step_loop(inv_model):
    m, ocfg, sd, *_ = inv_model
    from makeupdiffuse_amd.diffmk.cddim import MKDDIMSampler
    s = MKDDIMSampler(m)
    s.make_schedule(ddim_num_steps=10, verbose=False)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 4, 8, 8, generator=g).cuda()
    ctx = torch.randn(2, 77, 64, generator=g).cuda()
    uctx = torch.randn(2, 77, 64, generator=g).cuda()
    c = {'c_crossattn': [ctx], 'c_concat': None}
    uc = {'c_crossattn': [uctx], 'c_concat': None}
    for kw in ({}, dict(unconditional_guidance_scale=5.0, unconditional_conditioning=uc)):
        fast, out = s.encode(x0, c, 5, **kw)
        seen = []
        slow, _ = s.encode(x0, c, 5, callback=seen.append, **kw)
        assert seen == [0, 1, 2, 3, 4] and out['x_encoded'] is fast
        assert torch.equal(fast, slow), f'inversion {"CFG" if kw else "plain"}: in-library loop != step loop'
    sch = sampler.Schedule().make_ddim(10)
    ref = enc_ref.ddim_invert(sampler.make_eps_fn(sd, ocfg), sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev,
                              x0.cpu(), {'c_crossattn': [ctx.cpu()], 'c_concat': None}, 5)
    fast, _ = s.encode(x0, c, 5)
    check(fast, ref, 2e-2, 0.9995, 'inversion vs fp32 restatement over oracle.sampler.apply_model')


def test_get_z_and_invert_then_generate(inv_model):
    m, ocfg, sd, vcfg, vsd, esd = inv_model
    img = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    x = (img * 2 - 1).cuda()
    torch.manual_seed(123)
    z1 = m.get_z(x)
    torch.manual_seed(123)
    z2 = m.get_first_stage_encoding(m.encode_first_stage(x))
    torch.testing.assert_close(z1, z2, rtol=1e-6, atol=1e-6)
    post = m.encode_first_stage(x)
    assert torch.equal(post.mode(), post.mean) and post.parameters.shape == (2, 8, 8, 8)
    # invert_image -> generate_image vs the CPU composition of the restatements
    ctx = torch.randn(2, 77, 64, generator=torch.Generator().manual_seed(10))
    c = {'c_crossattn': [ctx.cuda()], 'c_concat_r': [img.cuda()], 'c_concat_s': [img.cuda()]}
    torch.manual_seed(7)
    inv = m.invert_image(img.cuda(), c)
    out = m.generate_image(inv, c)
    # each stage against its restatement, fed the device result of the stage before (the same draws of the posterior noise)
    torch.manual_seed(7)
    z_dev = m.get_z(x).cpu()
    torch.manual_seed(7)
    noise = torch.randn(2, 4, 8, 8)
    check(z_dev, enc_ref.latent(enc_ref.moments(esd, vcfg, img * 2 - 1), noise), 1.5e-2, 0.9997, 'get_z vs restatement')
    sch = sampler.Schedule(timesteps=m.t0, linear_start=m.linear_start, linear_end=m.linear_end).make_ddim(m.iter_finetune)
    eps_fn = sampler.make_eps_fn(sd, ocfg)
    inv_ref = enc_ref.ddim_invert(eps_fn, sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, z_dev,
                                  {'c_crossattn': [ctx], 'c_concat': None}, m.iter_finetune)
    # the latent of an image is small next to eps (|z| ~ 0.2): the inverted latent is dominated by the eps terms, so the budget is the
    # per-evaluation eps parity of the small net (2e-2 each) carried through the steps
    check(inv, inv_ref, 4e-2, 0.999, 'invert_image vs restatement')
    rec = sampler.reconstruct(eps_fn, sch, inv.cpu(), {'c_crossattn': [ctx], 'c_concat': [img]}, m.iter_finetune)
    img_ref = ((vae.decode_first_stage(vsd, vcfg, rec) + 1) / 2).clamp(0, 1)
    check(out, img_ref, 5e-2, 0.998, 'invert_image -> generate_image vs restatement')
