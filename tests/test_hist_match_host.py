"""CPU: the restatement tests/hist_match_ref.py reproduces what the reference's own functions recorded in
tests/golden/hist_match_ref.npz (tools/make_hist_golden.py) EXACTLY: tables, matched images, region masks, counts; losses within
1e-5 relative of the float64 mean over the golden matched image (fp32 sums of <= 2^22 non-negative terms: 1e-5 is about 8x the
pairwise-summation bound log2(N) 2^-24).  Plus the host side of the Python layer: argument validation, the runs/test.py switch, and
that the training entry points still raise."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import hist_match_ref as href
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import makeup_score as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'hist_match_ref.npz'))
CASES = (0, 1, 2)


def images(k):
    return (GOLD[f'c{k}_img_a'].astype(np.float32) / np.float32(65535.0), GOLD[f'c{k}_img_b'].astype(np.float32) / np.float32(65535.0))


def test_fixture_is_what_the_issue_asks_for():
    prov = json.loads(str(GOLD['provenance']))
    for key in ('c*_mask_*', 'c*_loss', 'c*_matched', 'c*_tables'):
        assert 'reference diffmk/' in prov[key]
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'hist_match_ref.npz')) < 512 * 1024
    sizes = [GOLD[f'c{k}_seg_a'].shape for k in CASES]
    assert sizes.count((128, 128)) >= 2 and (256, 256) in sizes
    assert max(int(GOLD[f'c{k}_count_a'][1]) for k in CASES if GOLD[f'c{k}_seg_a'].shape == (256, 256)) >= 15000
    for k in CASES:
        assert GOLD[f'c{k}_img_a'].dtype == np.uint16 and GOLD[f'c{k}_matched'].dtype == np.uint8 and GOLD[f'c{k}_tables'].dtype == np.uint8
        for s in 'ab':
            H, W = GOLD[f'c{k}_seg_{s}'].shape
            for lab in (4, 5):          # eyes >= 10 px from the border: the clipped box is never compared with the reference
                ys, xs = np.nonzero(GOLD[f'c{k}_seg_{s}'] == lab)
                assert ys.min() >= 10 and xs.min() >= 10 and ys.max() <= H - 11 and xs.max() <= W - 11
    # a region whose histogram is a single spike: case 1, image B under its lips
    b = GOLD['c1_img_b'][:, GOLD['c1_mask_b'][0] != 0]
    assert all(len(np.unique(b[c])) == 1 for c in range(3))


@pytest.mark.parametrize('k', CASES)
def test_restatement_region_masks_equal_the_reference(k):
    for s in 'ab':
        m = href.region_masks(GOLD[f'c{k}_seg_{s}'])
        for r, name in enumerate(href.REGIONS):
            assert np.array_equal(m[name], GOLD[f'c{k}_mask_{s}'][r]), (k, s, name)
            assert int(m[name].sum()) == int(GOLD[f'c{k}_count_{s}'][r])


@pytest.mark.parametrize('k', CASES)
def test_restatement_equals_the_reference_on_every_term(k):
    A, B = images(k)
    ma, mb = GOLD[f'c{k}_mask_a'], GOLD[f'c{k}_mask_b']
    for r in range(4):
        for d, (dst, ref, md, mr) in enumerate(((A, B, ma[r], mb[r]), (B, A, mb[r], ma[r]))):
            t = 2 * r + d
            matched, tables, loss, counts = href.histogram_match(dst, ref, md, mr)
            assert np.array_equal(tables, GOLD[f'c{k}_tables'][t]), (k, t)
            assert np.array_equal(matched, GOLD[f'c{k}_matched'][t].astype(np.float32)), (k, t)
            assert counts == (int(md.sum()), int(mr.sum()))
            l64 = href.loss_f64(dst, md, GOLD[f'c{k}_matched'][t])
            assert l64 > 0
            assert abs(float(loss) - l64) <= 1e-5 * l64, (k, t, float(loss), l64)
            assert abs(float(GOLD[f'c{k}_loss'][t]) - l64) <= 1e-5 * l64, (k, t, float(GOLD[f'c{k}_loss'][t]), l64)


def test_restatement_build_defined_cases():
    g = np.random.default_rng(3)
    dst, ref = g.random((3, 20, 30), dtype=np.float32), g.random((3, 20, 30), dtype=np.float32)
    full, none = np.ones((20, 30), np.uint8), np.zeros((20, 30), np.uint8)
    for md, mr in ((none, full), (full, none)):
        matched, tables, loss, counts = href.histogram_match(dst, ref, md, mr)
        assert not matched.any() and float(loss) == 0.0 and np.array_equal(tables, np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
    seg = np.ones((30, 30), np.uint8)
    seg[1:4, 2:6] = 4
    m = href.region_mask(seg, (1, 6), (4,), 10)
    assert m[:14, :16].sum() == 14 * 16 - 12 and m.sum() == 14 * 16 - 12          # clipped at the top-left corner
    assert href.region_mask(seg, (1, 6), (5,), 10).sum() == 0                    # no such eye: empty


def test_loss_makeup_expression_doubles_sr_skin():
    t = dict(sr_lip=1.0, rs_lip=2.0, sr_skin=4.0, rs_skin=100.0, sr_eye_left=8.0, rs_eye_left=16.0, sr_eye_right=32.0, rs_eye_right=64.0)
    assert href.loss_makeup(t) == ((1 + 2) + (4 + 4) + (8 + 16 + 32 + 64)) * 0.5
    assert href.loss_makeup(t, 2.0, 0.5, 7.0, 0.25) == ((2 + 4) + (2 + 2) + 120 * 0.25) * 0.5


# ---- the Python layer, host side ------------------------------------------------------------------------------------------------
def test_symbols_and_terms():
    for name in ('mkd_region_mask_from_labels', 'mkd_hist_match_scratch_bytes', 'mkd_hist_match', 'mkd_hist_match_launches'):
        assert name in mlib.SIGNATURES
    assert ms.TERMS == ('sr_lip', 'rs_lip', 'sr_skin', 'rs_skin', 'sr_eye_left', 'rs_eye_left', 'sr_eye_right', 'rs_eye_right')
    assert ms.REGIONS == href.REGIONS
    assert (ms.LIP_CLASSES, ms.SKIN_CLASSES, ms.FACE_CLASSES, ms.EYE_LEFT_CLASSES, ms.EYE_RIGHT_CLASSES, ms.EYE_MARGIN) == \
        (href.LIP, href.SKIN, href.FACE, href.EYE_LEFT, href.EYE_RIGHT, href.MARGIN)
    lib = mlib.load()
    assert lib.mkd_hist_match_scratch_bytes(0) == 0
    a, b = lib.mkd_hist_match_scratch_bytes(1), lib.mkd_hist_match_scratch_bytes(64)
    assert 0 < a < b and a % 256 == 0 and b % 256 == 0
    assert lib.mkd_hist_match_launches(1, 1) == 5 and lib.mkd_hist_match_launches(1, 0) == 4 and lib.mkd_hist_match_launches(0, 0) == 3


def test_argument_validation_and_no_cpu_path():
    img = torch.rand(2, 3, 16, 16)
    seg = torch.zeros(2, 16, 16, dtype=torch.uint8)
    with pytest.raises(mlib.MkdError):                    # host tensors: an error, never a CPU fallback
        ms.histogram_match(img, img, seg, seg)
    with pytest.raises(mlib.MkdError):
        ms.region_masks(seg)
    with pytest.raises(mlib.MkdError):
        ms.makeup_hist_terms(img, img, img, img, seg, seg)
    with pytest.raises(ValueError):
        ms.label_map(torch.zeros(16, 16))
    with pytest.raises(ValueError):
        ms.region_mask(seg, (64,))
    with pytest.raises(ValueError):
        ms.region_mask(seg, (1,), (4,), margin=-1)
    with pytest.raises(ValueError):
        ms.makeup_hist_terms(img, img, img, img, seg, seg, lambdas={'nose': 1.0})
    assert ms.label_map(torch.full((2, 1, 4, 4), 6.6)).tolist() == torch.full((2, 4, 4), 7, dtype=torch.uint8).tolist()
    assert tuple(ms.label_map(torch.zeros(2, 4, 5, 1)).shape) == (2, 4, 5)
    idx = ms._term_index(2, torch.device('cpu'))
    assert tuple(idx.shape) == (16, 4) and idx.dtype == torch.int32
    assert int(idx[:, :2].max()) == 7 and int(idx[:, 2:].max()) == 15 and int(idx.min()) == 0
    # row (2 r + d) B + b: sr reads SR[b] / R[b] under (src, ref) masks of region r, rs reads RS[b] / S[b] under (ref, src)
    assert idx[(2 * 1 + 0) * 2 + 1].tolist() == [1, 5, 5, 7] and idx[(2 * 1 + 1) * 2 + 1].tolist() == [3, 7, 7, 5]


def test_runs_test_parses_the_makeup_score_switch():
    spec = importlib.util.spec_from_file_location('runs_test_cli', os.path.join(ROOT, 'runs', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.build_parser().parse_args([]).makeup_score is False
    assert mod.build_parser().parse_args(['--makeup-score']).makeup_score is True
    b = mod.synthetic_batch(0, 2, 64, 8, with_makeup_seg=True)
    for k in ('nonmakeup_seg', 'makeup_seg'):
        assert b[k].dtype == torch.uint8 and all(int((b[k] == lab).sum()) > 0 for lab in (1, 4, 5, 7, 9))
    assert 'makeup_seg' not in mod.synthetic_batch(0, 2, 64, 8)


def test_training_entry_points_still_raise_and_the_weights_are_accepted():
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    from makeupdiffuse_amd.diffmk.makeups import BaseModel
    small = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                 hint_widths=(16, 16, 32, 32, 32, 32, 64), hint_channels=3, num_res_blocks=2, in_channels=4, use_spatial_transformer=True, legacy=False)
    m = BaseModel(control_stage_config={'params': small}, unet_config={'params': dict(small, out_channels=4)}, weight_loss_cycle=0.5,
                  weight_loss_makeup=2.0, weight_loss_idt=0.25, weight_loss_background=3.0, lambda_his_lip=1.0, lambda_his_skin_1=0.1,
                  lambda_his_skin_2=0.1, lambda_his_eye=1.0)
    assert (m.weight_loss_cycle, m.weight_loss_makeup, m.weight_loss_idt, m.weight_loss_background) == (0.5, 2.0, 0.25, 3.0)
    assert (m.lambda_his_lip, m.lambda_his_skin_1, m.lambda_his_skin_2, m.lambda_his_eye) == (1.0, 0.1, 0.1, 1.0)
    for fn in (m.shared_step, m.p_losses, m.forward):
        with pytest.raises(NotImplementedError):
            fn({})
    for name in ('get_msk_lip', 'get_msk_skin', 'get_msk_eye', 'criterionHis', 'p_loss_hist_lip', 'p_loss_hist_skin', 'p_loss_hist_eye',
                 'p_loss_makeup', 'p_loss_background', 'p_loss_idt', 'p_loss_cycle', 'validation_losses'):
        assert callable(getattr(m, name))
    a, b = torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    assert torch.allclose(m.p_loss_idt(a, b, b, a), (a - b).abs().mean())
    t = TestDiffuseModel(control_stage_config={'params': dict(small, hint_channels=6)}, unet_config={'params': dict(small, out_channels=4)})
    assert t.makeup_score is False and t.ref_seg_key == 'makeup_seg'
    assert TestDiffuseModel(control_stage_config={'params': dict(small, hint_channels=6)}, unet_config={'params': dict(small, out_channels=4)},
                            makeup_score=True).makeup_score is True
