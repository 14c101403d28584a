"""CPU: the face parser's host side.  The library's parameter table against the restatement's, refusals that must come before any
device call, the class remap tables, the model's plumbing on a duck-typed parser that returns given label maps, the command line,
and the fixture condition of the end-to-end label tests (tests/test_gpu_face_parser.py)."""
import ctypes as C
import dataclasses
import importlib.util
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import face_parser_ref as R
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import lib as mlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def _cfg_c(cfg):
    return fp.FaceParserConfig(**dataclasses.asdict(cfg)).to_c()


def _create(cfg):
    h = C.c_void_p()
    rc = mlib.load().mkd_parser_create(C.byref(_cfg_c(cfg)), C.byref(h))
    return rc, h


@pytest.mark.parametrize('cfg', [R.FULL, R.NARROW, dataclasses.replace(R.NARROW, blocks=(2, 2, 2, 2), n_classes=5)], ids=['full', 'narrow', 'narrow2'])
def test_parameter_table_equals_the_restatement(cfg):
    lib = mlib.load()
    rc, h = _create(cfg)
    assert rc == 0, lib.mkd_last_error()
    try:
        spec = R.param_spec(cfg)
        n = lib.mkd_parser_param_total(h)
        shp = (C.c_int64 * 4)()
        got = []
        for i in range(n):
            nd = lib.mkd_parser_param_shape(h, i, shp)
            got.append((lib.mkd_parser_param_name(h, i).decode(), tuple(int(shp[k]) for k in range(nd))))
        assert got == list(spec.items())                      # names, shapes AND the sorted order
        assert lib.mkd_parser_param_count(h) == R.param_count(cfg)
        assert lib.mkd_parser_param_name(h, n) is None and lib.mkd_parser_param_shape(h, -1, shp) < 0
    finally:
        lib.mkd_parser_destroy(h)
    p = fp.FaceParser(fp.FaceParserConfig(**dataclasses.asdict(cfg)), device='cpu')          # the Python class needs no device either
    assert p.expected_params() == spec and p.param_count() == R.param_count(cfg)
    p.close()


def test_full_config_is_upstreams_resnet18_bisenet():
    spec = R.param_spec(R.FULL)
    assert spec['cp.resnet.conv1.weight'] == (64, 3, 7, 7) and spec['cp.resnet.layer4.0.downsample.0.weight'] == (512, 256, 1, 1)
    assert 'cp.resnet.layer1.0.downsample.0.weight' not in spec and spec['ffm.convblk.conv.weight'] == (256, 256, 1, 1)
    assert spec['ffm.conv1.weight'] == (64, 256, 1, 1) and spec['conv_out.conv_out.weight'] == (19, 256, 1, 1)
    assert spec['cp.arm32.conv.conv.weight'] == (128, 512, 3, 3) and spec['cp.conv_avg.conv.weight'] == (128, 512, 1, 1)


@pytest.mark.parametrize('change', [dict(widths=(16, 36, 64, 128)), dict(widths=(12, 32, 64, 128)), dict(n_classes=1), dict(n_classes=33),
                                    dict(cp_channels=20), dict(ffm_channels=60), dict(blocks=(1, 0, 1, 1)), dict(bn_eps=0.0),
                                    dict(std=(0.2, 0.0, 0.2)), dict(widths=(136, 136, 136, 136))])
def test_create_refuses(change):
    rc, h = _create(dataclasses.replace(R.NARROW, **change))
    assert rc == ERR_ARG and not h.value and mlib.load().mkd_last_error()
    assert mlib.load().mkd_parser_create(None, C.byref(h)) == ERR_ARG
    assert mlib.load().mkd_parser_create(C.byref(_cfg_c(R.NARROW)), None) == ERR_ARG


def test_calls_refuse_before_any_device_call():
    """there is no device here: a refusal that came after a device call would be MKD_ERR_HIP (or a crash), not MKD_ERR_ARG"""
    lib = mlib.load()
    rc, h = _create(R.NARROW)
    assert rc == 0
    one = C.c_void_p(16)          # a non-null pointer that must never be followed
    try:
        for (B, H, W) in [(1, 48, 64), (1, 64, 48), (1, 1056, 64), (1, 64, 1056), (0, 64, 64), (65, 64, 64), (1, 80, 64), (-1, 64, 64)]:
            assert lib.mkd_parser_logits(h, one, B, H, W, one, None) == ERR_ARG
            assert lib.mkd_parser_parse(h, one, B, H, W, 64, 64, None, one, None, None) == ERR_ARG
        assert lib.mkd_parser_logits(None, one, 1, 64, 64, one, None) == ERR_ARG
        assert lib.mkd_parser_logits(h, None, 1, 64, 64, one, None) == ERR_ARG
        assert lib.mkd_parser_logits(h, one, 1, 64, 64, None, None) == ERR_ARG
        assert lib.mkd_parser_parse(h, one, 1, 64, 64, 64, 64, None, None, None, None) == ERR_ARG
        assert lib.mkd_parser_parse(h, one, 1, 64, 64, 0, 64, None, one, None, None) == ERR_ARG
        assert lib.mkd_parser_parse(h, one, 1, 64, 64, 64, -3, None, one, None, None) == ERR_ARG
        assert lib.mkd_parser_parse(h, one, 1, 64, 64, 64, 64, None, one, None, None) == -3          # valid arguments, not finalized: MKD_ERR_STATE
        assert lib.mkd_parser_launches(h) == 0 and lib.mkd_parser_flops(h, 64, 64) > 0 and lib.mkd_parser_flops(h, 48, 64) == 0
        # weights: unknown / wrongly shaped -> MKD_ERR_ARG; the training-only keys are not an error
        w = np.zeros((16, 3, 7, 7), np.float32)
        ld = lambda name, a: lib.mkd_parser_load_weight(h, name, a.ctypes.data_as(C.c_void_p), a.ndim, (C.c_int64 * 4)(*a.shape))
        assert ld(b'cp.resnet.conv1.weight', w) == 0
        assert ld(b'cp.resnet.conv1.weight', w[:8]) == ERR_ARG and ld(b'cp.resnet.conv1.weight', w.reshape(16, 147)) == ERR_ARG
        assert ld(b'cp.resnet.conv2.weight', w) == ERR_ARG
        assert ld(b'conv_out16.conv.conv.weight', w) == 0 and ld(b'conv_out32.conv_out.weight', w) == 0
        assert ld(b'cp.resnet.bn1.num_batches_tracked', np.zeros((), np.float32)) == 0
        assert lib.mkd_parser_finalize(h) == -5 and b'conv_out.conv.bn.bias' in lib.mkd_last_error()          # MKD_ERR_MISSING names the first missing tensor
    finally:
        lib.mkd_parser_destroy(h)
    # the head alone
    ok = dict(logits=one, batch=1, nc=19, h8=8, w8=8, P_h=64, P_w=64, out_h=64, out_w=64, labels=one)
    def head(**kw):
        a = dict(ok, **kw)
        return lib.mkd_parse_labels(a['logits'], 64, 8, 1, 64 * 19, a['batch'], a['nc'], a['h8'], a['w8'], a['P_h'], a['P_w'], a['out_h'], a['out_w'],
                                    None, a['labels'], None)
    for bad in (dict(logits=None), dict(labels=None), dict(batch=0), dict(nc=1), dict(nc=33), dict(h8=0), dict(w8=0), dict(P_h=0), dict(out_h=0),
                dict(out_w=0), dict(out_h=-5)):
        assert head(**bad) == ERR_ARG, bad
    # the single kernels
    assert lib.mkd_channel_gate(one, 12, 1, 4, 12, one, None, 4, 1, None, None, 0, 0, one, None) == ERR_ARG          # C % 8
    assert lib.mkd_channel_gate(one, 16, 1, 0, 16, one, None, 4, 1, None, None, 0, 0, one, None) == ERR_ARG          # no pixel
    assert lib.mkd_channel_gate(one, 16, 1, 4, 16, one, None, 4, 3, None, None, 0, 0, one, None) == ERR_ARG          # activation code
    assert lib.mkd_gate_apply_bf16(one, 16, one, 3, one, 16, one, 16, 1, 4, 4, 16, 0, None) == ERR_ARG               # mode
    assert lib.mkd_gate_apply_bf16(one, 16, one, 0, None, 16, one, 16, 1, 4, 4, 16, 0, None) == ERR_ARG              # mode 0 without its vector
    assert lib.mkd_gate_apply_bf16(one, 16, one, 2, None, 0, one, 16, 1, 4, 4, 16, 2, None) == ERR_ARG               # u
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.mkd_parser_stem(one, one, one, m3, m3, one, one, 1, 48, 64, 16, None) == ERR_ARG
    assert lib.mkd_parser_stem(one, one, one, m3, m3, one, one, 1, 64, 64, 136, None) == ERR_ARG


def test_python_layer_needs_a_device_for_compute():
    with pytest.raises(mlib.MkdError):
        fp.parse_labels(torch.zeros(1, 19, 8, 8), (64, 64))
    with pytest.raises(ValueError):
        fp.parse_labels(torch.zeros(19, 8, 8), (64, 64))
    with pytest.raises(ValueError):
        fp._check_lut([0] * 18, 19)


def test_remap_tables():
    names = fp.CLASS_NAMES
    assert len(names) == 19 and len(fp.LUT_SEG) == 19 and len(fp.LUT_PREPROCESS) == 19
    assert max(fp.LUT_SEG) <= 13 and max(fp.LUT_PREPROCESS) <= 13 and min(fp.LUT_SEG + fp.LUT_PREPROCESS) >= 0
    assert list(fp.LUT_PREPROCESS) == [0, 1, 2, 3, 4, 5, 0, 11, 12, 0, 6, 8, 7, 9, 13, 0, 0, 10, 0] == R.LUT_PREPROCESS
    seg = dict(zip(names, fp.LUT_SEG))
    assert {seg['u_lip'], seg['l_lip']} == {7, 9} and seg['mouth'] == 11 and seg['hair'] == 12 and seg['skin'] == 1
    assert seg['nose'] == 6 and seg['neck'] == 13 and seg['l_ear'] == seg['r_ear'] == 8
    assert all(seg[k] == 0 for k in ('bg', 'eye_g', 'ear_r', 'neck_l', 'cloth', 'hat'))
    assert (seg['l_brow'], seg['r_brow'], seg['l_eye'], seg['r_eye']) == (2, 3, 4, 5)
    # what the consumers select: the score's regions, the background classes, the face box
    from makeupdiffuse_amd import makeup_score as ms
    assert set(ms.LIP_CLASSES) == {7, 9} and set(ms.SKIN_CLASSES) == {1, 6, 13} and 8 not in set(ms.FACE_CLASSES) | set(fp.FACE_CLASSES)


# ---- model plumbing on a fake parser ------------------------------------------------------------------------------------------------

class FakeParser:
    """duck-typed: parse() returns the label maps it was given, resized by the head's nearest rule, and records its calls"""

    def __init__(self, maps):
        self.maps, self.calls = maps, []

    def parse(self, img01, out_size=None, lut=None, return_logits=False):
        B, _, H, W = img01.shape
        oh, ow = (H, W) if out_size is None else ((out_size, out_size) if isinstance(out_size, int) else tuple(out_size))
        self.calls.append((tuple(img01.shape), (oh, ow), tuple(lut) if lut is not None else None))
        m = self.maps[:B]
        ys = (torch.arange(oh) * m.shape[1]) // oh
        xs = (torch.arange(ow) * m.shape[2]) // ow
        return m[:, ys][:, :, xs].contiguous()


NET = dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64, num_res_blocks=2, in_channels=4,
           use_spatial_transformer=True, legacy=False)


def _model(**kw):
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    return TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=[16, 16, 32, 32, 32, 32, 64])},
                            unet_config={'params': dict(NET, out_channels=4)}, **kw)


def test_model_fills_label_maps_only_when_absent():
    maps = torch.zeros(2, 128, 128, dtype=torch.uint8); maps[:, 32:96, 40:80] = 1; maps[1, 70:80, 50:70] = 7
    fake = FakeParser(maps)
    m = _model(face_parser=fake, parse_size=128)
    assert m.parse_size == 128 and m.parser_lut == tuple(fp.LUT_SEG)
    img = torch.rand(2, 3, 64, 64)
    batch = {'src_img': img, 'ref_img': img}
    m._fill_segs(batch)
    assert 'makeup_seg' not in batch and batch['nonmakeup_seg'].shape == (2, 64, 64) and batch['nonmakeup_seg'].dtype == torch.uint8
    assert fake.calls == [((2, 3, 128, 128), (64, 64), tuple(fp.LUT_SEG))]          # parsed at parse_size, labels at the image size
    assert torch.equal(batch['nonmakeup_seg'], maps[:, ::2, ::2])
    m._fill_segs(batch, ref=True)
    assert len(fake.calls) == 2 and 'makeup_seg' in batch                            # the source's map was there: only the reference is parsed
    mine = torch.full((2, 64, 64), 5, dtype=torch.uint8)
    batch2 = {'src_img': img, 'ref_img': img, 'nonmakeup_seg': mine}
    m._fill_segs(batch2)
    assert batch2['nonmakeup_seg'] is mine and len(fake.calls) == 2                  # label maps the caller brings win
    m128 = _model(face_parser=fake, parse_size=64)                                   # images already at parse size go in as they are
    m128._fill_segs({'src_img': img, 'ref_img': img})
    assert fake.calls[-1][0] == (2, 3, 64, 64)
    with pytest.raises(ValueError):
        _model(parse_size=100)
    with pytest.raises(ValueError):
        _model().parse_images(img)


def test_without_a_parser_the_key_errors_stand():
    m = _model()
    assert m.face_parser is None
    img = torch.rand(2, 3, 64, 64)
    batch = {'src_img': img, 'ref_img': img, 'txt_emb': torch.zeros(2, 77, 64)}
    m._fill_segs(batch, ref=True)
    assert 'nonmakeup_seg' not in batch and 'makeup_seg' not in batch
    with pytest.raises(KeyError, match='nonmakeup_seg'):
        m.transfer_regions(batch, {'lip': 'ref_img'})
    with pytest.raises(KeyError, match='nonmakeup_seg'):
        m.makeup_hist(batch, img, img)
    m.first_stage_encoder = True
    with pytest.raises(KeyError, match='nonmakeup_seg'):
        m.background_latents(batch, img)


Cropped = namedtuple('Cropped', 'img01 labels u8')


def host_box(labels, classes):
    """stand-in for the device's box of mkd_region_mask_from_labels: (row min, row max, col min, col max), (INT_MAX, -1, INT_MAX, -1) when empty"""
    m = torch.zeros_like(labels, dtype=torch.bool)
    for c in classes:
        m |= labels == int(c)
    rows, cols = m.any(1).nonzero().flatten().tolist(), m.any(0).nonzero().flatten().tolist()
    return (rows[0], rows[-1], cols[0], cols[-1]) if rows else (2 ** 31 - 1, -1, 2 ** 31 - 1, -1)


@pytest.mark.parametrize('H,W', [(300, 200), (200, 300)])
def test_find_boxes_maps_a_blob_back(H, W):
    from makeupdiffuse_amd import photo
    S = 64
    # a skin blob over photo rows 90..149, columns 60..99, seen through the squash to S x S
    r0, r1, c0, c1 = 90, 149, 60, 99
    lab = torch.zeros(1, S, S, dtype=torch.uint8)
    ys, xs = (torch.arange(S) * H) // S, (torch.arange(S) * W) // S          # photo pixel that parse pixel (y, x) shows
    inside = ((ys >= r0) & (ys <= r1))[:, None] & ((xs >= c0) & (xs <= c1))[None, :]
    lab[0][inside] = 1
    lab[0, 0, 0] = 8                                                           # an ear pixel: not a face class
    fake = FakeParser(lab)
    seen = []
    def resize(photos, boxes, size):
        seen.append((boxes, size))
        return Cropped(torch.zeros(len(photos), 3, size, size), None, None)
    photo_t = torch.zeros(H, W, 3, dtype=torch.uint8)
    (box,) = fp.find_boxes(fake, [photo_t], grow=0.0, parse_size=S, resize=resize, box_of=host_box)
    assert seen == [([(0, 0, W, H)], S)] and fake.calls[0][1] == (S, S)
    # grow 0: the square about the blob's box, as grow_square_box makes it from the blob's own extent (within one parse pixel)
    want = photo.grow_square_box((r0, r1, c0, c1), H, W, 0.0)
    step = max(-(-H // S), -(-W // S))
    assert all(abs(a - b) <= step for a, b in zip(box, want)), (box, want)
    x0, y0, side, _ = box
    assert x0 <= c0 + step and y0 <= r0 + step and x0 + side > c1 - step and y0 + side > r1 - step and x0 >= 0 and y0 >= 0 and x0 + side <= W and y0 + side <= H
    grown = fp.find_boxes(fake, [photo_t], grow=1.0, parse_size=S, resize=resize, box_of=host_box)[0]
    assert grown[2] >= side and grown[0] + grown[2] <= W and grown[1] + grown[3] <= H
    with pytest.raises(ValueError, match='photo 1'):
        fp.find_boxes(FakeParser(torch.cat([lab, torch.zeros_like(lab)])), [photo_t, photo_t], parse_size=S, resize=resize, box_of=host_box)


def test_transfer_photos_without_boxes_needs_a_parser():
    p = [torch.zeros(80, 80, 3, dtype=torch.uint8)]
    with pytest.raises(ValueError, match='boxes'):
        _model().transfer_photos(p, p)
    with pytest.raises(ValueError, match='boxes'):
        _model().transfer_photos(p, p, [(0, 0, 80, 80)])


def test_runs_test_leaves_the_parser_off_by_default():
    spec = importlib.util.spec_from_file_location('runs_test_cli_parser', os.path.join(ROOT, 'runs', 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args([])
    assert a.face_parser is None
    assert mod.build_parser().parse_args(['--face-parser', 'random']).face_parser == 'random'
    assert mod.synthetic_seg(0, 64).shape == (64, 64)          # runs without the flag keep their synthetic label maps


# ---- the fixture condition of the end-to-end label tests ---------------------------------------------------------------------------

def _near_tie_share(cfg, seed, B, H, W):
    sd = R.init_state_dict(cfg, seed)
    x = R.make_images(B, H, W, seed=B)
    Lr = R.logits(sd, cfg, x)
    E = (R.logits_bf16(sd, cfg, x) - Lr).abs().max().item()
    top2 = R.upsample(Lr, H, W).topk(2, dim=1).values
    return ((top2[:, 0] - top2[:, 1]) <= 4 * E).float().mean().item(), E


@pytest.mark.parametrize('B,H,W', [(2, 64, 64), (3, 64, 96)])
@pytest.mark.parametrize('nc', [19, 5])
@pytest.mark.parametrize('blocks', [(1, 1, 1, 1), (2, 2, 2, 2)])
def test_fixture_condition_narrow(blocks, nc, B, H, W):
    """The restatement alone must allow the GPU label test's bounds: with a device error D <= 2 E, only pixels whose top-two margin
    is <= 2 D <= 4 E may change label, and those are at most 1 % of the map for the committed seeds and images."""
    share, E = _near_tie_share(dataclasses.replace(R.NARROW, blocks=blocks, n_classes=nc), R.SEEDS[(blocks, nc)], B, H, W)
    assert E > 0 and share <= 0.01, (share, E)


def test_fixture_condition_full_size():
    share, E = _near_tie_share(R.FULL, R.SEEDS['full'], 1, 512, 512)
    assert E > 0 and share <= 0.01, (share, E)


def test_head_restatement_on_known_maps():
    """the numpy head: identity at h8 == P, first maximum on ties, the nearest rule of the final resize"""
    lg = np.zeros((1, 3, 2, 2), np.float32); lg[0, 1, 0, 0] = 1.0; lg[0, 2, 1, 1] = 1.0
    assert R.head_np(lg, 2, 2, 2, 2).tolist() == [[[1, 0], [0, 2]]]
    assert R.head_np(lg, 2, 2, 4, 4)[0, :2, :2].tolist() == [[1, 1], [1, 1]] and R.head_np(lg, 2, 2, 1, 1).tolist() == [[[1]]]
    assert R.head_np(lg, 2, 2, 2, 2, lut=[9, 8, 7]).tolist() == [[[8, 9], [9, 7]]]
    up = R.head_np(lg, 4, 4, 4, 4)
    assert up[0, 0, 0] == 1 and up[0, 3, 3] == 2 and up.shape == (1, 4, 4)
