"""-m gpu: the pixel-space background paste on the model class: TestDiffuseModel(paste_background=True).log_results and
transfer_regions(paste_outside=True), bit for bit against the engine call on the unpasted decode and against the source expression."""
import numpy as np
import pytest
import torch

import paste_background_ref as pref
from gpu_util import DEV
from makeupdiffuse_amd import regions as rg
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from oracle import nets, vae

pytestmark = pytest.mark.gpu

NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])      # f = 8: 8 x 8 latent -> 64 x 64
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))
B = 2


def build(**kw):
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, ddim_steps=2,
                         unconditional_guidance_scale=9, **kw)
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m.load_state_dict({**nets.init_state_dict(OCFG, seed=31), **vae.init_state_dict(vcfg, seed=32)})
    m.cuda(0)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(34))
    m.save_images = False
    return m


@pytest.fixture(scope='module')
def plain():
    return build()


@pytest.fixture(scope='module')
def pasting():
    return build(paste_background=True, paste_feather=0)


def face_label_map():
    """background 0 around skin (1) with hair (12) on top, eyes (4, 5), lips (7, 9) and teeth (11); sample 1 is shifted"""
    seg = torch.zeros(B, 64, 64, dtype=torch.uint8)
    for b in range(B):
        o = 3 * b
        seg[b, 2 + o:10 + o, 10:54] = 12
        seg[b, 10 + o:56 + o, 12:52] = 1
        seg[b, 20 + o:24 + o, 18:26] = 4
        seg[b, 20 + o:24 + o, 38:46] = 5
        seg[b, 40 + o:43 + o, 24:40] = 7
        seg[b, 43 + o:44 + o, 28:36] = 11
        seg[b, 44 + o:47 + o, 24:40] = 9
    return seg


@pytest.fixture(scope='module')
def batch():
    g = torch.Generator().manual_seed(96)
    return {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g),
            'ref_lip': torch.rand(B, 3, 64, 64, generator=g), 'txt_emb': torch.randn(B, 77, 64, generator=g),
            'nonmakeup_seg': face_label_map(), 'x_T': torch.randn(B, 4, 8, 8, generator=g)}


def source_expression(control_src):
    """((control_src + 1) / 2) * 2 - 1, one rounding per operation (CPU)"""
    s = control_src.float().cpu()
    return ((s + 1.0) / 2.0) * 2.0 - 1.0


def same(a, b):
    return np.array_equal(pref.bits(a.detach().cpu().numpy()), pref.bits(b.detach().cpu().numpy()))


def test_log_results_pastes_every_decoded_entry(pasting, batch):
    m = pasting
    names = ('samples', 'samples_cfg_scale_9.00')
    for feather in (0, 3):
        m.paste_feather = feather
        try:
            log = m.log_results(batch, 0, x_T=batch['x_T'].to(DEV))
        finally:
            m.paste_feather = 0
        alpha = log['mask_pixel']
        assert tuple(alpha.shape) == (B, 1, 64, 64)
        want_alpha = pref.alpha_from_labels(batch['nonmakeup_seg'].numpy(), (0, 11, 12), 1, feather)
        assert np.array_equal(pref.bits(alpha.cpu().numpy()), pref.bits(want_alpha))
        for name in names:
            decoded = m.decode_first_stage(log[name + '_latent'])                 # the *_latent entries are untouched: the unpasted decode
            want, a = m.engine.paste_background(decoded, log['control_src'], seg=batch['nonmakeup_seg'], classes=(0, 11, 12),
                                                feather=feather, return_alpha=True)
            assert same(log[name], want) and same(a, alpha), (name, feather)
            assert same(log[name], torch.from_numpy(pref.paste(decoded.cpu().numpy(), log['control_src'].cpu().numpy(), want_alpha)))
            keep = (alpha == 1.0).expand(-1, 3, -1, -1).cpu()
            assert 0.1 < float(keep.float().mean()) < 0.7
            assert same(log[name].cpu()[keep], source_expression(log['control_src'])[keep]), (name, feather)
            face = (alpha == 0.0).expand(-1, 3, -1, -1).cpu()
            assert face.any() and not torch.equal(log[name].cpu()[face], source_expression(log['control_src'])[face])
    assert not torch.equal(log['samples_latent'], log['samples_cfg_scale_9.00_latent'])


def test_option_off_is_the_model_without_it(plain, pasting, batch):
    x_T = batch['x_T'].to(DEV)
    base = plain.log_results(batch, 0, x_T=x_T)
    assert 'mask_pixel' not in base
    pasting.paste_background = False
    try:
        off = pasting.log_results(batch, 0, x_T=x_T)
    finally:
        pasting.paste_background = True
    assert list(off) == list(base)
    for k in base:
        assert torch.equal(off[k], base[k]), k
    on = pasting.log_results(batch, 0, x_T=x_T)
    assert [k for k in on if k != 'mask_pixel'] == list(base)
    for k in base:
        assert torch.equal(on[k], base[k]) == (k not in ('samples', 'samples_cfg_scale_9.00')), k


def test_missing_inputs(pasting, batch):
    with pytest.raises(KeyError):
        pasting.log_results({k: v for k, v in batch.items() if k != 'nonmakeup_seg'}, 0)


def test_makeup_score_is_taken_on_the_pasted_image(pasting, batch):
    m = pasting
    b2 = dict(batch, makeup_seg=face_label_map())
    m.makeup_score, m.paste_feather = True, 3             # (a feather: the band reaches into the skin, so the two scores below differ)
    try:
        log = m.log_results(b2, 0, x_T=batch['x_T'].to(DEV))
    finally:
        m.makeup_score, m.paste_feather = False, 0
    ref = m.get_origin_img_input(b2, m.ref_img_key)
    assert torch.equal(log['makeup_hist'], m.makeup_hist(b2, log['samples'], ref))
    assert not torch.equal(log['makeup_hist'], m.makeup_hist(b2, m.decode_first_stage(log['samples_latent']), ref))


def test_transfer_regions_paste_outside(plain, pasting, batch):
    x_T = batch['x_T'].to(DEV)
    refs = {'lip': 'ref_lip'}
    un = plain.transfer_regions(batch, refs, base='source', x_T=x_T)
    out = plain.transfer_regions(batch, refs, base='source', x_T=x_T, paste_outside=True)
    assert torch.equal(out['samples_latent'], un['samples_latent']) and 'mask_pixel' not in out
    region = rg.user_region_masks(batch['nonmakeup_seg'].to(DEV), ('lip',)).amax(0).cpu().bool()        # [B,H,W]
    assert region.any() and not region.all()
    assert np.array_equal(out['mask_outside'].cpu().numpy()[:, 0], (~region).numpy().astype(np.float32))
    src_pm1 = batch['src_img'] * 2.0 - 1.0
    outside = (~region)[:, None].expand(-1, 3, -1, -1)
    inside = region[:, None].expand(-1, 3, -1, -1)
    got = out['samples'].cpu()
    assert same(got[outside], source_expression(src_pm1)[outside])
    # inside a region the weight is 0 and the seven operations leave clamp(((t + 1) / 2) * 2 - 1) of the unpasted decode t: its bits are
    # the restatement's, and it is clamp(t) up to the rounding of t + 1 (at most 2^-23 for t + 1 in [2, 4), less below)
    t = un['samples'].cpu()
    zero = np.zeros((B, 1, 64, 64), np.float32)
    assert same(got[inside], torch.from_numpy(pref.paste(t.numpy(), src_pm1.numpy(), zero))[inside])
    assert float((got[inside] - t.clamp(-1, 1)[inside]).abs().max()) <= 2.0 ** -23
    # both options: the background classes first, then everything outside the regions
    both = pasting.transfer_regions(batch, refs, base='source', x_T=x_T, paste_outside=True)
    assert torch.equal(both['samples_latent'], un['samples_latent'])
    assert np.array_equal(pref.bits(both['mask_pixel'].cpu().numpy()),
                          pref.bits(pref.alpha_from_labels(batch['nonmakeup_seg'].numpy(), (0, 11, 12), 1, 0)))
    step1 = pref.paste(t.numpy(), src_pm1.numpy(), both['mask_pixel'].cpu().numpy())
    step2 = pref.paste(step1, src_pm1.numpy(), out['mask_outside'].cpu().numpy())
    assert same(both['samples'], torch.from_numpy(step2))
    only_bg = pasting.transfer_regions(batch, refs, base='source', x_T=x_T)
    assert same(only_bg['samples'], torch.from_numpy(step1)) and 'mask_outside' not in only_bg
    with pytest.raises(ValueError):
        plain.transfer_regions(batch, refs, base='ref', x_T=x_T, paste_outside=True)


def test_interpolate_is_pasted(pasting, batch):
    m = pasting
    b2 = dict(batch, ref_img2=batch['ref_lip'])
    out = m.interpolate(b2, [0.0, 1.0], x_T=batch['x_T'].to(DEV))
    assert tuple(out['samples'].shape) == (2 * B, 3, 64, 64)
    seg = batch['nonmakeup_seg'].repeat_interleave(2, 0)
    src = (batch['src_img'] * 2.0 - 1.0).repeat_interleave(2, 0)
    alpha = pref.alpha_from_labels(seg.numpy(), (0, 11, 12), 1, 0)
    assert np.array_equal(pref.bits(out['mask_pixel'].cpu().numpy()), pref.bits(alpha))
    decoded = m.decode_first_stage(out['samples_latent'])
    assert same(out['samples'], torch.from_numpy(pref.paste(decoded.cpu().numpy(), src.numpy(), alpha)))
