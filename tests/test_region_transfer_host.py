"""CPU: region-wise transfer from several references (BUILD-DEFINED) - the numpy restatement of the weight definition
has the properties the definition promises, the three new C entries refuse bad arguments before they touch a device, and
TestDiffuseModel.transfer_regions / the runs/test.py switch validate their arguments."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import region_transfer_ref as rref
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import regions as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MKD_ERR_ARG = -1


def random_masks(rng, K, B, H, W, p=0.3):
    m = (rng.random((K, B, H, W)) < p).astype(np.uint8)
    m[rng.random(m.shape) < 0.05] = 200                       # any non-zero value is "inside"
    return m


# ---- the weight definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 3, 7])
@pytest.mark.parametrize('f,rho', [(8, 0), (8, 1), (4, 4), (4, 0)])
def test_planes_sum_to_one(K, f, rho):
    rng = np.random.default_rng(10 * K + rho)
    B, H, W = 2, 48, 80
    masks = random_masks(rng, K, B, H, W)
    w = rref.region_weights(masks, f, rho)
    assert w.shape == (B, K + 1, H // f, W // f) and w.dtype == np.float32 and (w >= 0).all()
    s = w.astype(np.float64).sum(1)
    assert np.abs(s - 1.0).max() <= K * 2.0 ** -24
    if rho == 0:                                              # a_k = cnt / f^2 with f^2 a power of two: every step is exact
        assert np.array_equal(s, np.ones_like(s))
    st = rng.random((B, K)).astype(np.float32)
    ws = rref.region_weights(masks, f, rho, st)
    assert np.abs(ws.astype(np.float64).sum(1) - 1.0).max() <= K * 2.0 ** -24
    assert np.array_equal(ws[:, 1:], st[:, :, None, None] * w[:, 1:])


def test_priority_resolves_overlap():
    K, B, H, W, f = 3, 1, 16, 16, 8
    masks = np.zeros((K, B, H, W), np.uint8)
    masks[0, 0, :8, :8] = 1                                   # region 0: the top-left block
    masks[1, 0, :8, :] = 1                                    # region 1 overlaps it: owns only the top-right block
    masks[2, 0] = 1                                           # region 2 covers everything: owns what is left
    w = rref.region_weights(masks, f, 0)
    assert np.array_equal(w[0, 1], [[1, 0], [0, 0]]) and np.array_equal(w[0, 2], [[0, 1], [0, 0]])
    assert np.array_equal(w[0, 3], [[0, 0], [1, 1]]) and np.array_equal(w[0, 0], np.zeros((2, 2)))
    cnt = rref.owned_counts(masks, f)
    assert cnt.sum() == H * W and cnt[1].sum() == 64
    swapped = rref.region_weights(masks[[2, 1, 0]], f, 0)     # the all-covering mask first: the others own nothing
    assert np.array_equal(swapped[0, 1], np.ones((2, 2))) and not swapped[0, 2:].any()


def test_wholly_owned_window_and_zero_strength():
    rng = np.random.default_rng(3)
    B, H, W = 2, 64, 64
    for f, rho in ((8, 0), (8, 1), (8, 4), (4, 4)):
        masks = random_masks(rng, 2, B, H, W)
        masks[0, :, :, :] = 0
        masks[0, 0] = 1                                       # sample 0: region 0 owns every pixel, so every window
        w = rref.region_weights(masks, f, rho)
        assert np.array_equal(w[0, 1], np.ones_like(w[0, 1])) and not w[0, 0].any() and not w[0, 2].any()
        z = rref.region_weights(masks, f, rho, np.zeros((B, 2), np.float32))
        assert np.array_equal(z[:, 0], np.ones_like(z[:, 0])) and not z[:, 1:].any()
    masks = np.zeros((2, 1, 16, 16), np.uint8)                # two regions that tile the image: exact at feather 0
    masks[0, 0, :, :5] = 1; masks[1, 0, :, 3:] = 1
    w = rref.region_weights(masks, 8, 0)
    assert not w[0, 0].any() and np.array_equal(w[0, 1] + w[0, 2], np.ones((2, 2), np.float32))


def test_window_clamps_to_the_edge():
    cnt = np.arange(6, dtype=np.int64).reshape(1, 1, 2, 3)
    s = rref.window_sums(cnt, 1)                              # 3 x 3 window on a 2 x 3 grid: rows clamp on both sides
    rows = np.array([[0, 0, 1], [0, 1, 1]]); cols = np.array([[0, 0, 1], [0, 1, 2], [1, 2, 2]])
    want = np.array([[sum(cnt[0, 0, r, c] for r in rows[y] for c in cols[x]) for x in range(3)] for y in range(2)])
    assert np.array_equal(s[0, 0], want)


# ---- C ABI: bad arguments come back as MKD_ERR_ARG without a device ------------------------------------------------------------
def test_new_entries_refuse_bad_arguments_without_a_device():
    lib = mlib.load()
    for name in ('mkd_prepare_regions', 'mkd_region_weights', 'mkd_region_blend_bf16', 'mkd_debug_hint_embedding'):
        assert name in mlib.SIGNATURES
    assert lib.mkd_abi_version() == 1
    buf = (C.c_char * 4096)()                                  # stands for device memory: a refused call never reads it
    p = C.c_void_p(C.addressof(buf))
    rw = lambda masks, K, B, H, W, f, rho, out: lib.mkd_region_weights(masks, K, B, H, W, f, rho, None, out, None)
    assert rw(None, 1, 1, 8, 8, 8, 0, p) == MKD_ERR_ARG and rw(p, 1, 1, 8, 8, 8, 0, None) == MKD_ERR_ARG
    for K in (0, 8):
        assert rw(p, K, 1, 8, 8, 8, 0, p) == MKD_ERR_ARG
    for rho in (-1, 5):
        assert rw(p, 1, 1, 8, 8, 8, rho, p) == MKD_ERR_ARG
    for H, W, f in ((12, 8, 8), (8, 12, 8), (8, 8, 0), (128, 128, 65), (0, 8, 8)):
        assert rw(p, 1, 1, H, W, f, 0, p) == MKD_ERR_ARG
    assert rw(p, 1, 0, 8, 8, 8, 0, p) == MKD_ERR_ARG
    assert rw(p, 7, 1, 128, 64, 1, 0, p) == MKD_ERR_ARG       # 7 x 128 x 64 block counts do not fit the LDS staging
    assert b'region_weights' in lib.mkd_last_error()
    tab = (C.c_void_p * 8)(*([C.addressof(buf)] * 8))
    rb = lambda e, w, out, B, hw, Cn, R: lib.mkd_region_blend_bf16(e, w, out, B, hw, Cn, R, None)
    assert rb(None, p, p, 1, 4, 8, 2) == MKD_ERR_ARG and rb(tab, None, p, 1, 4, 8, 2) == MKD_ERR_ARG and rb(tab, p, None, 1, 4, 8, 2) == MKD_ERR_ARG
    for R in (0, 9):
        assert rb(tab, p, p, 1, 4, 8, R) == MKD_ERR_ARG
    assert rb(tab, p, p, 1, 4, 12, 2) == MKD_ERR_ARG and rb(tab, p, p, 0, 4, 8, 2) == MKD_ERR_ARG and rb(tab, p, p, 1, 0, 8, 2) == MKD_ERR_ARG
    hole = (C.c_void_p * 8)(C.addressof(buf), None)
    assert rb(hole, p, p, 1, 4, 8, 2) == MKD_ERR_ARG
    pr = lambda ctx, hints, n, w, cx: lib.mkd_prepare_regions(ctx, 1, 8, 8, hints, n, w, cx, None, 0, None)
    assert pr(None, tab, 2, p, p) == MKD_ERR_ARG
    for n in (0, 9, -1):                                       # refused on the arguments alone, whatever the context is
        assert pr(p, tab, n, p, p) == MKD_ERR_ARG
    assert pr(p, None, 2, p, p) == MKD_ERR_ARG and pr(p, tab, 2, None, p) == MKD_ERR_ARG and pr(p, tab, 2, p, None) == MKD_ERR_ARG
    assert pr(p, hole, 2, p, p) == MKD_ERR_ARG
    assert lib.mkd_prepare_regions(p, 0, 8, 8, tab, 2, p, p, None, 0, None) == MKD_ERR_ARG
    assert lib.mkd_debug_hint_embedding(None, p, None) == MKD_ERR_ARG


# ---- Python layer ----------------------------------------------------------------------------------------------------------------
SMALL = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
             hint_widths=(16, 16, 32, 32, 32, 32, 64), hint_channels=6, num_res_blocks=2, in_channels=4, use_spatial_transformer=True, legacy=False)


def test_regions_module_validation():
    assert rg.ordered(['skin', 'eye']) == ('eye', 'skin') and rg.ordered({'lip': 'a'}) == ('lip',) and rg.PRIORITY == ('eye', 'lip', 'skin')
    for bad in (['nose'], [], ['lip', 'lip']):
        with pytest.raises(ValueError):
            rg.ordered(bad)
    st = rg.strength_rows({'lip': 0.5, 'eye': [0.0, 1.0]}, ('eye', 'lip', 'skin'), 2)
    assert st.dtype == torch.float32 and st.tolist() == [[0.0, 0.5, 1.0], [1.0, 0.5, 1.0]]
    assert rg.strength_rows(None, ('lip',), 2) is None
    for bad in ({'skin': 1.0}, {'lip': [1.0, 2.0, 3.0]}, {'lip': -0.1}, {'lip': float('nan')}):
        with pytest.raises(ValueError):
            rg.strength_rows(bad, ('lip',), 2)
    seg = torch.zeros(2, 16, 16, dtype=torch.uint8)
    with pytest.raises(mlib.MkdError):                        # host tensors: an error, never a CPU fallback
        rg.region_weights_from_seg(seg, ['lip'])
    with pytest.raises(mlib.MkdError):
        rg.region_weights(torch.zeros(1, 2, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        rg.region_weights_from_seg(seg, ['lip'], feather=5)


def test_transfer_regions_argument_validation():
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    m = TestDiffuseModel(control_stage_config={'params': SMALL}, unet_config={'params': dict(SMALL, out_channels=4)})
    img = torch.rand(2, 3, 64, 64)
    batch = {'src_img': img, 'ref_img': img, 'lip_ref': img, 'txt_emb': torch.zeros(2, 77, 64), 'nonmakeup_seg': torch.zeros(2, 64, 64, dtype=torch.uint8)}
    with pytest.raises(ValueError):
        m.transfer_regions(batch, {'nose': 'lip_ref'})
    with pytest.raises(ValueError):
        m.transfer_regions(batch, {})
    with pytest.raises(ValueError):
        m.transfer_regions(batch, {'lip': 'lip_ref'}, base='both')
    with pytest.raises(ValueError):
        m.transfer_regions(batch, {'lip': 'lip_ref'}, feather=5)
    with pytest.raises(ValueError):
        m.transfer_regions(batch, {'lip': 'lip_ref'}, strengths={'eye': 1.0})
    with pytest.raises(KeyError):                             # a missing label map, as makeup_hist reports it
        m.transfer_regions({k: v for k, v in batch.items() if k != 'nonmakeup_seg'}, {'lip': 'lip_ref'})
    with pytest.raises(KeyError):
        m.transfer_regions(batch, {'lip': 'no_such_key'})
    with pytest.raises(mlib.MkdError):                        # valid arguments, no device: loud
        m.transfer_regions(batch, {'lip': 'lip_ref'})


def test_runs_test_parses_the_region_switches():
    spec = importlib.util.spec_from_file_location('runs_test_cli_regions', os.path.join(ROOT, 'runs', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args([])
    assert a.region_refs is None and a.region_strength is None and a.region_feather == 1
    a = mod.build_parser().parse_args(['--region-refs', 'lip=makeup/a.png,eye=makeup/b.png', '--region-strength', 'lip=0.7', '--region-feather', '2'])
    assert mod.parse_region_map(a.region_refs) == {'lip': 'makeup/a.png', 'eye': 'makeup/b.png'}
    assert mod.parse_region_map(a.region_strength, float) == {'lip': 0.7} and a.region_feather == 2
    assert mod.parse_region_map(None) == {}
    for bad in ('lip', 'lip=a,lip=b'):
        with pytest.raises(ValueError):
            mod.parse_region_map(bad)
