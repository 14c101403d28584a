"""-m gpu: TestDiffuseModel.transfer_photos on a small model at S = 64: photos of different sizes in, the same photos out, bit for bit
the chain of the existing calls (sample_log, decode, paste_source) between the two photo calls, and the source's own bytes wherever
the background paste keeps the source."""
import numpy as np
import pytest
import torch

import photo_ref as pr
import vae_encoder_ref as enc_ref
from gpu_util import DEV
from makeupdiffuse_amd import photo
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from oracle import nets, vae

pytestmark = pytest.mark.gpu

NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])      # f = 8: 8 x 8 latent -> 64 x 64
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))
S = 64
SRC_SIZES, REF_SIZES = ((150, 203), (97, 130)), ((120, 90), (70, 64))
SRC_BOXES, REF_BOXES = [(30, 10, 130, 130), (0, 5, 90, 88)], [(5, 20, 80, 80), (0, 0, 64, 64)]


@pytest.fixture(scope='module')
def model():
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True,
                         ddim_steps=2, unconditional_guidance_scale=9)
    m.load_state_dict({**nets.init_state_dict(OCFG, seed=31), **vae.init_state_dict(vcfg, seed=32), **enc_ref.init_state_dict(vcfg, seed=33)})
    m.cuda(0)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(34))
    m.save_images = False
    return m


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(77)
    rand = lambda hw: torch.randint(0, 256, (hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    segs = []
    for (H, W), (x0, y0, bw, bh) in zip(SRC_SIZES, SRC_BOXES):           # background 0 around a face (1) with hair (12) on top, in the box
        s = torch.zeros(H, W, dtype=torch.uint8)
        s[y0 + bh // 8: y0 + bh // 4, x0 + bw // 4: x0 + 3 * bw // 4] = 12
        s[y0 + bh // 4: y0 + 7 * bh // 8, x0 + bw // 4: x0 + 3 * bw // 4] = 1
        s[y0 + bh // 2: y0 + bh // 2 + 6, x0 + bw // 3: x0 + bw // 3 + 10] = 7
        segs.append(s)
    return dict(src=[rand(s) for s in SRC_SIZES], ref=[rand(s) for s in REF_SIZES], segs=segs,
                batch={'txt_emb': torch.randn(2, 77, 64, generator=g)}, x_T=torch.randn(2, 4, 8, 8, generator=g))


def by_hand(m, d, feather):
    """the chain transfer_photos is documented to run, from the existing calls and the two photo calls"""
    src_dev = [p.to(DEV) for p in d['src']]
    cs = photo.crop_resize(src_dev, SRC_BOXES, S, labels=[s.to(DEV) for s in d['segs']])
    cr = photo.crop_resize([p.to(DEV) for p in d['ref']], REF_BOXES, S)
    src, ref = cs.img01, cr.img01
    ctx = d['batch']['txt_emb'].to(DEV)
    cond = {'c_concat': [torch.cat((src, ref), 1)], 'c_crossattn': [ctx]}
    extra = {'x_T': d['x_T'].to(DEV)}
    if m.fix_background:
        x0, mask = m.background_latents({m.seg_key: cs.labels}, src)
        extra.update(x0=x0, mask=mask)
    if m.unconditional_guidance_scale > 1.0:
        extra.update(unconditional_guidance_scale=float(m.unconditional_guidance_scale),
                     unconditional_conditioning={'c_concat': cond['c_concat'], 'c_crossattn': [m.get_unconditional_conditioning(2)]})
    lat, _ = m.sample_log(cond=cond, batch_size=2, ddim=True, ddim_steps=m.ddim_steps, eta=m.ddim_eta, **extra)
    img = m.decode_first_stage(lat)
    if m.paste_background:
        img, _ = m.paste_source({m.seg_key: cs.labels}, img, src * 2.0 - 1.0)
    out = [p.clone() for p in src_dev]
    photo.paste_photos(out, SRC_BOXES, img, src, feather)
    return out, cs, img


@pytest.mark.parametrize('fix,paste,scale,sampler', [(False, False, 9, 'ddim'), (True, True, 9, 'ddim'), (False, True, 1.0, 'dpmpp')])
def test_transfer_photos_is_the_chain_of_the_calls(model, data, fix, paste, scale, sampler):
    m = model
    m.fix_background, m.paste_background, m.unconditional_guidance_scale, m.sampler = fix, paste, scale, sampler
    try:
        m.reset_conditioning_cache()
        torch.manual_seed(123)                     # fix_background draws (the posterior sample, the blend's noise rows) from the default generator
        got = m.transfer_photos(data['src'], data['ref'], SRC_BOXES, REF_BOXES, src_segs=data['segs'], feather=3, x_T=data['x_T'], size=S,
                                batch=data['batch'])
        m.reset_conditioning_cache()
        torch.manual_seed(123)
        want, cs, img = by_hand(m, data, 3)
    finally:
        m.fix_background, m.paste_background, m.unconditional_guidance_scale, m.sampler = False, False, 9, 'ddim'
    assert len(got) == 2
    for i, (g, w, p, box) in enumerate(zip(got, want, data['src'], SRC_BOXES)):
        assert g.dtype == torch.uint8 and g.device.type == 'cuda' and tuple(g.shape) == tuple(p.shape)
        g, w, p = g.cpu().numpy(), w.cpu().numpy(), p.numpy()
        assert np.array_equal(g, w), f'photo {i}: {int((g != w).sum())} bytes differ from the chain of the calls'
        x0, y0, bw, bh = box
        inside = np.zeros(p.shape[:2], bool)
        inside[y0:y0 + bh, x0:x0 + bw] = True
        assert np.array_equal(g[~inside], p[~inside]) and (g[inside] != p[inside]).mean() > 0.3
        # the device chain against the restatement of the two photo calls around the device's decode
        u8 = pr.crop_resize_u8(p, box, S)
        assert np.array_equal(cs.img01[i].cpu().numpy().view(np.uint32), pr.img01(u8).view(np.uint32))
        assert np.array_equal(g, pr.paste(p, box, img[i].cpu().numpy(), pr.img01(u8), 3))


def test_kept_background_is_the_source_photo(model, data):
    """paste_background keeps background (0) and hair (12): a photo pixel whose four model-resolution neighbours are all kept gets its
    own bytes back, the face does not"""
    m = model
    m.paste_background, m.background_classes = True, (0, 12)
    try:
        m.reset_conditioning_cache()
        got = m.transfer_photos(data['src'], data['ref'], SRC_BOXES, REF_BOXES, src_segs=data['segs'], feather=0, x_T=data['x_T'], size=S,
                                batch=data['batch'])
    finally:
        m.paste_background, m.background_classes = False, (0, 11, 12)
    for g, p, seg, box in zip(got, data['src'], data['segs'], SRC_BOXES):
        g, p = g.cpu().numpy(), p.numpy()
        x0, y0, bw, bh = box
        kept = np.isin(pr.crop_labels(seg.numpy(), box, S), (0, 12))
        ya, yb, _ = pr._axis(bh, S)
        xa, xb, _ = pr._axis(bw, S)
        all_kept = kept[ya][:, xa] & kept[ya][:, xb] & kept[yb][:, xa] & kept[yb][:, xb]
        region, was = g[y0:y0 + bh, x0:x0 + bw], p[y0:y0 + bh, x0:x0 + bw]
        assert all_kept.mean() > 0.2 and (~all_kept).mean() > 0.2
        assert np.array_equal(region[all_kept], was[all_kept])
        assert (region[~all_kept] != was[~all_kept]).mean() > 0.3


def test_transfer_photos_needs_label_maps_for_the_background_options(model, data):
    model.paste_background = True
    try:
        with pytest.raises(KeyError):
            model.transfer_photos(data['src'], data['ref'], SRC_BOXES, REF_BOXES, size=S, batch=data['batch'])
    finally:
        model.paste_background = False
