"""The pixel-space background paste without a device: the numpy restatement the GPU tests compare with (paste_background_ref.py)
against the reference's own three lines, the exactness of its weights, the 8-bit round trip the harness test relies on, and the
validation that needs no device."""
import numpy as np
import pytest
import torch

import paste_background_ref as pref
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.imageio import grid_to_uint8

NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]


def build_model(**kw):
    return TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                            unet_config={'params': dict(NET, out_channels=4)}, ddim_steps=2, **kw)


def test_restatement_equals_the_references_three_lines_bit_for_bit():
    """reference Fixbackground.get_target (diffmk/makeup_teacher.py:254-262) as torch CPU ops, hard mask over background 0, teeth 11, hair 12"""
    g = torch.Generator().manual_seed(11)
    B, H, W = 3, 37, 53
    nonmakeup_img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    target = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    seg = torch.randint(0, 15, (B, H, W), generator=g, dtype=torch.uint8)
    _bkgrd = ((seg == 0) | (seg == 11) | (seg == 12)).float().unsqueeze(1)
    assert 0.05 < float(_bkgrd.mean()) < 0.5
    want = _bkgrd * ((nonmakeup_img + 1) / 2) + (1 - _bkgrd) * ((target + 1) / 2)
    want = want * 2.0 - 1.0
    want = want.clamp(-1, 1)
    alpha = pref.alpha_from_labels(seg.numpy(), (0, 11, 12), 1, 0)
    assert np.array_equal(alpha, _bkgrd.numpy())
    got = pref.paste(target.numpy(), nonmakeup_img.numpy(), alpha)
    assert np.array_equal(pref.bits(got), pref.bits(want.numpy()))


def test_weights_are_exact_fractions():
    rng = np.random.default_rng(3)
    B, H, W = 2, 9, 13
    for f in range(1, 9):
        labels = rng.integers(0, 15, (B, f * H, f * W), dtype=np.uint8)
        labels[rng.random(labels.shape) < 0.02] = 200                      # labels >= 64 never match
        full = np.full_like(labels, 12)
        none = np.full_like(labels, 3)
        for rho in range(0, 17):
            D = (2 * rho + 1) ** 2 * f * f
            a = pref.alpha_from_labels(labels, (0, 11, 12), f, rho)
            assert a.shape == (B, 1, H, W) and a.dtype == np.float32
            n = a.astype(np.float64) * D
            assert np.array_equal(np.round(n)[:, 0], pref.window_sums(pref.class_counts(labels, (0, 11, 12), f), rho))
            assert np.abs(n - np.round(n)).max() <= 2.0 ** -24 * D             # alpha D is the integer S up to the division's one rounding
            assert (a >= 0).all() and (a <= 1).all()
            assert np.array_equal(pref.alpha_from_labels(full, (0, 11, 12), f, rho), np.ones((B, 1, H, W), np.float32))
            assert not pref.alpha_from_labels(none, (0, 11, 12), f, rho).any()
    # the window sum against a direct double loop (clamped indices), on one small case
    cnt = rng.integers(0, 5, (1, 5, 7)).astype(np.int64)
    for rho in (1, 3, 16):
        want = np.zeros_like(cnt)
        for y in range(5):
            for x in range(7):
                want[0, y, x] = sum(cnt[0, min(max(y + dy, 0), 4), min(max(x + dx, 0), 6)]
                                    for dy in range(-rho, rho + 1) for dx in range(-rho, rho + 1))
        assert np.array_equal(pref.window_sums(cnt, rho), want)


def test_a_pasted_source_pixel_is_saved_as_the_source_byte():
    """for every byte value k: s = k/255 * 2 - 1 (control_src of an 8-bit image) and its pasted form ((s + 1) / 2) * 2 - 1 reach the same
    byte through save_local's arithmetic.  The harness test compares PNG bytes on the strength of this."""
    k = torch.arange(256, dtype=torch.float32)
    s = (k / 255.0) * 2.0 - 1.0
    pasted = torch.from_numpy(pref.paste(np.zeros((1, 1, 1, 256), np.float32), s.numpy().reshape(1, 1, 1, 256), np.ones((1, 1, 1, 256), np.float32)))
    assert np.array_equal(pref.bits(pasted.numpy()), pref.bits((((s + 1) / 2) * 2 - 1).numpy().reshape(1, 1, 1, 256)))
    a = grid_to_uint8(s.reshape(1, 1, 256).expand(3, 1, 256))
    b = grid_to_uint8(pasted.reshape(1, 1, 256).expand(3, 1, 256))
    assert int((a != b).sum()) == 0


def test_constructor_and_keyword_validation():
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            build_model(paste_feather=bad)
    m = build_model(paste_background=True, paste_feather=16)
    assert m.paste_background is True and m.paste_feather == 16 and m.fix_background is False
    d = build_model()
    assert d.paste_background is False and d.paste_feather == 0
    batch = {'src_img': torch.zeros(1, 3, 64, 64), 'ref_img': torch.zeros(1, 3, 64, 64), 'lip': torch.zeros(1, 3, 64, 64),
             'nonmakeup_seg': torch.zeros(1, 64, 64, dtype=torch.uint8), 'txt_emb': torch.zeros(1, 77, 64)}
    with pytest.raises(ValueError, match="base='source'"):
        d.transfer_regions(batch, {'lip': 'lip'}, base='ref', paste_outside=True)
    with pytest.raises(ValueError, match='first stage'):                       # no decoder: nothing to paste into
        d.transfer_regions(batch, {'lip': 'lip'}, base='source', paste_outside=True)
    with pytest.raises(ValueError, match='first stage'):
        m.log_results(batch, 0)
