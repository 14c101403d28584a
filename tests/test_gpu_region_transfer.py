"""-m gpu: region-wise makeup transfer from several references (BUILD-DEFINED): the weights kernel against its numpy
restatement bit for bit, the blend kernel against fp32 torch, the engine wiring bit for bit (one-hot planes, the cached embedding,
re-preparing, the plan key), the ten-step trajectory against the restated oracle loop, and TestDiffuseModel.transfer_regions.

The issue's single-eps-against-the-oracle test is left out as the issue provides: with the seeded weights no input with
control_scales <= 8 moves the oracle's eps by the 6e-2 precondition (measured 1.2e-3 .. 2.7e-3); test 3(c) carries the
spatial check."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hist_match_ref as href
import region_transfer_ref as rref
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import regions as rg
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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the weights kernel has the restatement's bits -----------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(64, 64), (48, 80)])
def test_weights_kernel_equals_the_numpy_restatement_bit_for_bit(H, W):
    rng = np.random.default_rng(H + W)
    B = 3
    for K in (1, 3, 7):
        masks = (rng.random((K, B, H, W)) < 0.35).astype(np.uint8)
        masks[rng.random(masks.shape) < 0.05] = 255                        # any non-zero byte is inside
        masks[:, 0, : H // 2] = 1                                          # sample 0: every mask claims the top half (priority decides)
        if K > 1:
            masks[K - 1, 1] = 1                                            # sample 1: the last region owns whatever the others leave
        strength = (2.0 * rng.random((B, K))).astype(np.float32)           # above 1 too: the base weight then clamps at 0
        md = torch.from_numpy(masks).to(DEV)
        sd_ = torch.from_numpy(strength).to(DEV)
        for f in (8, 4):
            for rho in (0, 1, 4):
                for st_np, st_dev in ((None, None), (strength, sd_)):
                    out = rg.region_weights(md, f, rho, st_dev)
                    ref = rref.region_weights(masks, f, rho, st_np)
                    got = out.cpu().numpy()
                    assert got.shape == ref.shape == (B, K + 1, H // f, W // f)
                    assert np.array_equal(bits(got), bits(ref)), f'K {K} f {f} feather {rho} strength {st_np is not None}'
    # a mask base that is not 4-byte aligned takes the byte-wise load path: the same bits
    K, f, rho = 3, 8, 1
    masks = (rng.random((K, B, H, W)) < 0.4).astype(np.uint8)
    flat = torch.zeros(K * B * H * W + 8, dtype=torch.uint8, device=DEV)
    flat[1:1 + K * B * H * W] = torch.from_numpy(masks).to(DEV).flatten()
    shifted = flat[1:1 + K * B * H * W].view(K, B, H, W)
    assert shifted.data_ptr() % 4 == 1 and shifted.is_contiguous()
    got = rg.region_weights(shifted, f, rho).cpu().numpy()
    assert np.array_equal(bits(got), bits(rref.region_weights(masks, f, rho)))


# ---- 2. the blend kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cn', [64, 320])
@pytest.mark.parametrize('R', [1, 2, 5, 8])
def test_blend_kernel_against_fp32_torch(R, Cn):
    lib = L()
    g = torch.Generator().manual_seed(100 * R + Cn)
    B = 3
    for hw in (64, 128):
        es = [torch.randn(B, hw, Cn, generator=g).to(DEV).to(torch.bfloat16).contiguous() for _ in range(R)]
        w = torch.randn(B, R, hw, generator=g).to(DEV)                      # arbitrary fp32 weights, negative ones included
        tab = (C.c_void_p * R)(*[e.data_ptr() for e in es])
        outs = []
        for _ in range(2):
            out = torch.full((B, hw, Cn), float('nan'), device=DEV, dtype=torch.bfloat16)
            assert lib.mkd_region_blend_bf16(tab, P(w), P(out), B, hw, Cn, R, None) == 0
            sync()
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), 'two runs differ'
        ref = rref.blend_f32(es, w)
        bound = 2.0 ** -8 * rref.blend_abs(es, w)
        err = (outs[0].float() - ref).abs()
        assert torch.isfinite(outs[0].float()).all() and (err <= bound).all(), f'R {R} C {Cn} hw {hw}: worst {float((err - bound).max()):.3e} over the bound'
        alias = es[0].clone()                                               # out aliasing e[0]
        tab_a = (C.c_void_p * R)(*([alias.data_ptr()] + [e.data_ptr() for e in es[1:]]))
        assert lib.mkd_region_blend_bf16(tab_a, P(w), P(alias), B, hw, Cn, R, None) == 0
        sync()
        assert torch.equal(alias.view(torch.int16), outs[0].view(torch.int16)), 'in place != out of place'


# ---- 3. engine wiring, bit for bit -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    sd = nets.init_state_dict(OCFG, seed=31)
    eng = MkdEngine(NetConfig(hint_channels=6, model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2,
                              context_dim=64, hint_widths=tuple(HINT_WIDTHS)))
    eng.load_state_dict(sd)
    yield eng, sd
    eng.close()


def wiring_inputs(B=3, R=3, seed=80):
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(B, 3, 64, 64, generator=g)
    hints = [torch.cat((src, torch.rand(B, 3, 64, 64, generator=g)), 1).to(DEV) for _ in range(R)]
    return dict(hints=hints, ctx=torch.randn(B, 77, 64, generator=g).to(DEV), uctx=torch.randn(B, 77, 64, generator=g).to(DEV),
                x=torch.randn(B, 4, 8, 8, generator=g).to(DEV), t=torch.tensor([801, 401, 41][:B] if B <= 3 else [401] * B).to(DEV),
                w=torch.rand(B, R, 8, 8, generator=g).to(DEV))


def test_engine_one_hot_planes_equal_the_plain_prepare(small):
    eng, _ = small
    I = wiring_inputs()
    B, R = 3, 3
    plain = []
    for r in range(R):
        eng.prepare(I['hints'][r], I['ctx'])
        plain.append(eng.eps(I['x'], I['t']).clone())
    launches = eng.eps_launches()
    assert not torch.equal(plain[0], plain[1]) and not torch.equal(plain[1], plain[2])
    for r in range(R):                                                       # (a) plane r is 1 everywhere
        w = torch.zeros(B, R, 8, 8, device=DEV); w[:, r] = 1.0
        eng.prepare_regions(I['hints'], w, I['ctx'])
        assert torch.equal(eng.eps(I['x'], I['t']), plain[r]), f'plane {r} = 1 is not prepare(hint {r})'
        assert eng.eps_launches() == launches
    pick = [2, 0, 1]                                                         # (b) one reference per SAMPLE
    w = torch.zeros(B, R, 8, 8, device=DEV)
    for b, r in enumerate(pick):
        w[b, r] = 1.0
    eng.prepare_regions(I['hints'], w, I['ctx'])
    got = eng.eps(I['x'], I['t']).clone()
    mixed = torch.stack([I['hints'][r][b] for b, r in enumerate(pick)])
    eng.prepare(mixed, I['ctx'])
    assert torch.equal(got, eng.eps(I['x'], I['t'])), 'per-sample one-hot planes != the per-sample mixed hint'


def test_engine_embedding_replanning_and_plan_key(small):
    eng, _ = small
    lib = L()
    I = wiring_inputs()
    B, R, hw, Cn = 3, 3, 64, 64
    embs = []
    for r in range(R):                                                       # (c) the cached embedding = the stand-alone blend of the three
        eng.prepare(I['hints'][r], I['ctx'])
        embs.append(eng.debug_hint_embedding().clone())
    eng.prepare_regions(I['hints'], I['w'], I['ctx'])
    got = eng.debug_hint_embedding().clone()
    tab = (C.c_void_p * R)(*[e.data_ptr() for e in embs])
    want = torch.empty_like(got)
    assert lib.mkd_region_blend_bf16(tab, P(I['w']), P(want), B, hw, Cn, R, None) == 0
    sync()
    assert tuple(got.shape) == (B, 8, 8, Cn) and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not torch.equal(got, embs[0])
    # (d) new weights, same R: another result, the same plan (launch counts, device memory)
    e1 = eng.eps(I['x'], I['t']).clone()
    n_step, n_cfg, n_eps, mem = eng.step_launches(), eng.step_launches(True, True), eng.eps_launches(), eng.device_bytes()
    w2 = I['w'].flip(1).contiguous()
    eng.prepare_regions(I['hints'], w2, I['ctx'])
    e2 = eng.eps(I['x'], I['t']).clone()
    assert not torch.equal(e1, e2)
    assert (eng.step_launches(), eng.step_launches(True, True), eng.eps_launches(), eng.device_bytes()) == (n_step, n_cfg, n_eps, mem)
    eng.prepare_regions(I['hints'], I['w'], I['ctx'])
    assert torch.equal(eng.eps(I['x'], I['t']), e1)
    # (e) interpolation before and after a regions call: the same bits
    alpha = torch.tensor([0.0, 0.3, 1.0], device=DEV)
    eng.prepare(I['hints'][0], I['ctx'], hint2=I['hints'][1], alpha=alpha)
    before = eng.eps(I['x'], I['t']).clone()
    emb_before = eng.debug_hint_embedding().clone()
    eng.prepare_regions(I['hints'], I['w'], I['ctx'])
    eng.eps(I['x'], I['t'])
    eng.prepare(I['hints'][0], I['ctx'], hint2=I['hints'][1], alpha=alpha)
    assert torch.equal(eng.debug_hint_embedding().view(torch.int16), emb_before.view(torch.int16))
    assert torch.equal(eng.eps(I['x'], I['t']), before)
    eng.prepare(I['hints'][0], I['ctx'])                                     # ... and the plain path after both
    eng2 = eng.eps(I['x'], I['t']).clone()
    eng.prepare_regions(I['hints'], torch.cat([torch.ones(B, 1, 8, 8), torch.zeros(B, R - 1, 8, 8)], 1).to(DEV), I['ctx'])
    assert torch.equal(eng.eps(I['x'], I['t']), eng2)
    with pytest.raises(ValueError):
        eng.prepare_regions(I['hints'], I['w'][:, :2], I['ctx'])
    with pytest.raises(ValueError):
        eng.prepare_regions([], I['w'], I['ctx'])


def test_debug_hint_embedding_needs_prepared_conditioning():
    eng = MkdEngine(NetConfig(hint_channels=6, model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2,
                              context_dim=64, hint_widths=tuple(HINT_WIDTHS)))
    out = torch.empty(8, device=DEV, dtype=torch.bfloat16)
    assert L().mkd_debug_hint_embedding(eng._ctx, P(out), None) == -3       # MKD_ERR_STATE
    eng.close()


# ---- 5. ten-step trajectory against the restated oracle loop -----------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 9.0])
def test_ten_step_trajectory_vs_oracle(small, scale):
    eng, sd = small
    B, R, S = 2, 3, 10
    I = wiring_inputs(B=B, R=R, seed=90)
    w = I['w'] / I['w'].sum(1, keepdim=True)                                 # a convex blend per latent pixel
    sch = sampler.Schedule().make_ddim(S)
    args = (sch.ddim_timesteps, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas)
    cpu = lambda t: t.cpu()
    hints_c, w_c, ctx_c, uctx_c, x_c = [cpu(t) for t in I['hints']], cpu(w), cpu(I['ctx']), cpu(I['uctx']), cpu(I['x'])
    guided = scale != 1.0
    dup = (lambda t: torch.cat([t, t])) if guided else (lambda t: t)
    ctx_dev = torch.cat([I['uctx'], I['ctx']]) if guided else I['ctx']
    # regions
    eng.prepare_regions([dup(t) for t in I['hints']], dup(w), ctx_dev)
    out_g = eng.sample(I['x'], *args, cfg_scale=scale, use_graph=True).clone()
    out_e = eng.sample(I['x'], *args, cfg_scale=scale, use_graph=False).clone()
    assert torch.equal(out_g, out_e), 'graph replay != eager loop'
    cond = {'c_crossattn': [ctx_c], 'c_concat_regions': hints_c, 'region_weights': w_c}
    uc = {'c_crossattn': [uctx_c], 'c_concat_regions': hints_c, 'region_weights': w_c} if guided else None
    ref = sampler.sample(rref.make_eps_fn(sd, OCFG), sampler.Schedule(), x_c, cond, S, unconditional_guidance_scale=scale,
                         unconditional_conditioning=uc)
    r_reg, c_reg = metrics(out_g, ref)
    # the single-reference trajectory of the same inputs: the parent's path, measured in the same run
    eng.prepare(dup(I['hints'][0]), ctx_dev)
    out_1 = eng.sample(I['x'], *args, cfg_scale=scale, use_graph=True)
    cond1 = {'c_crossattn': [ctx_c], 'c_concat': [hints_c[0]]}
    uc1 = {'c_crossattn': [uctx_c], 'c_concat': [hints_c[0]]} if guided else None
    ref1 = sampler.sample(sampler.make_eps_fn(sd, OCFG), sampler.Schedule(), x_c, cond1, S, unconditional_guidance_scale=scale,
                          unconditional_conditioning=uc1)
    r_one, c_one = metrics(out_1, ref1)
    print(f'[parity] 10-step latent, guidance {scale}: regions rel-L2 {r_reg:.4e} cos {c_reg:.6f}; single reference rel-L2 {r_one:.4e} cos {c_one:.6f}')
    assert c_reg >= 0.99
    assert r_reg <= 2.0 * r_one


# ---- 6. the model class ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mm():
    sd = nets.init_state_dict(OCFG, seed=31)
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, ddim_steps=5, unconditional_guidance_scale=9)
    m.load_state_dict({**sd, **vae.init_state_dict(vcfg, seed=32)})
    m.cuda(0)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(34))
    m.save_images = False
    return m


def face_label_map(B=2):
    """rectangles of skin (1), neck (13), eyes (4, 5) and upper lip (7) on background; sample 1 is shifted"""
    seg = torch.zeros(B, 64, 64, dtype=torch.uint8)
    for b in range(B):
        o = 3 * b
        seg[b, 8 + o:52 + o, 12:52] = 1
        seg[b, 52 + o:60 + o, 20:44] = 13
        seg[b, 20 + o:24 + o, 18:26] = 4
        seg[b, 20 + o:24 + o, 38:46] = 5
        seg[b, 40 + o:45 + o, 24:40] = 7
    return seg


def restated_masks(seg, regs):
    per = [href.region_masks(s.numpy()) for s in seg]
    pick = lambda m, r: (m['eye_left'] | m['eye_right']) if r == 'eye' else m[r]
    return np.stack([np.stack([pick(m, r) for m in per]) for r in regs]).astype(np.uint8)


def test_transfer_regions_on_the_model_class(mm):
    m = mm
    g = torch.Generator().manual_seed(95)
    B = 2
    seg = face_label_map(B)
    batch = {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g),
             'ref_lip': torch.rand(B, 3, 64, 64, generator=g), 'ref_eye': torch.rand(B, 3, 64, 64, generator=g),
             'ref_skin': torch.rand(B, 3, 64, 64, generator=g), 'txt_emb': torch.randn(B, 77, 64, generator=g), 'nonmakeup_seg': seg}
    x_T = torch.randn(B, 4, 8, 8, generator=g).to(DEV)
    refs = {'lip': 'ref_lip', 'skin': 'ref_skin', 'eye': 'ref_eye'}          # (any order: the planes follow eye > lip > skin)
    strengths = {'lip': 0.7, 'eye': [1.0, 0.25]}
    out = m.transfer_regions(batch, refs, strengths=strengths, feather=1, x_T=x_T)
    regs = ('eye', 'lip', 'skin')
    masks = restated_masks(seg, regs)
    assert all(masks[k].any() for k in range(3)) and (masks[0] & masks[2]).any()      # the eye boxes do overlap the skin
    st = np.array([[1.0, 0.7, 1.0], [0.25, 0.7, 1.0]], np.float32)
    want = rref.region_weights(masks, 8, 1, st)
    assert tuple(out['weights'].shape) == (B, 4, 8, 8) and np.array_equal(bits(out['weights'].cpu().numpy()), bits(want))
    assert tuple(out['samples_latent'].shape) == (B, 4, 8, 8) and tuple(out['samples'].shape) == (B, 3, 64, 64)
    assert torch.isfinite(out['samples_latent']).all() and torch.isfinite(out['samples']).all()
    # every strength 0 on the reference base: the ordinary single-reference sampling, bit for bit (plain and guided)
    zero = {r: 0.0 for r in regs}
    _, c = m.get_input(batch, m.first_stage_key)
    cond = {'c_concat': [c['c_concat'][0]], 'c_crossattn': [c['c_crossattn'][0]]}
    plains = {}
    for scale in (1.0, 9.0):
        kw = {}
        if scale != 1.0:
            kw = dict(unconditional_guidance_scale=scale,
                      unconditional_conditioning={'c_concat': cond['c_concat'], 'c_crossattn': [m.get_unconditional_conditioning(B)]})
        plain, _ = m.sample_log(cond=cond, batch_size=B, ddim=True, ddim_steps=m.ddim_steps, eta=0.0, x_T=x_T, **kw)
        plains[scale] = plain
        z = m.transfer_regions(batch, refs, strengths=zero, base='ref', x_T=x_T, unconditional_guidance_scale=scale)
        assert torch.equal(z['samples_latent'], plain), f'strength 0 != single-reference sampling (guidance {scale})'
        assert np.array_equal(z['weights'][:, 0].cpu().numpy(), np.ones((B, 8, 8), np.float32)) and not z['weights'][:, 1:].any()
        full = m.transfer_regions(batch, refs, x_T=x_T, unconditional_guidance_scale=scale)
        assert metrics(full['samples_latent'], plain)[0] > 1e-4               # the references do act
    src_base = m.transfer_regions(batch, refs, strengths=zero, base='source', x_T=x_T)
    assert not torch.equal(src_base['samples_latent'], plains[1.0])          # src||src as the base is another hint
    # the sampler attribute is honoured
    ddim = m.transfer_regions(batch, refs, x_T=x_T)
    m.sampler = 'dpmpp'
    try:
        dpm = m.transfer_regions(batch, refs, x_T=x_T)
    finally:
        m.sampler = 'ddim'
    assert torch.isfinite(dpm['samples_latent']).all() and not torch.equal(dpm['samples_latent'], ddim['samples_latent'])
    with pytest.raises(KeyError):
        m.transfer_regions({k: v for k, v in batch.items() if k != 'nonmakeup_seg'}, refs, x_T=x_T)
