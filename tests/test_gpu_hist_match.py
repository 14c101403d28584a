"""-m gpu: region-wise histogram matching and the makeup score on the device (mkd_region_mask_from_labels, mkd_hist_match,
makeupdiffuse_amd.makeup_score, BaseModel.validation_losses, TestDiffuseModel(makeup_score=True)).

tests/golden/hist_match_ref.npz was written by the reference's own functions (tools/make_hist_golden.py); the device's tables,
matched images, region masks and counts must EQUAL it, the loss is within 1e-5 relative of the float64 mean.  Build-defined cases
(empty region, clipped eye box, non-square) are compared with the restatement tests/hist_match_ref.py.

Bounds: a device loss against the float64 mean of the same matched image: 1e-5 relative.  Where the expected value is the
restatement's own fp32 loss (the batch / model tests), 2e-5: each side is within 1e-5 of the float64 mean."""
import os

import numpy as np
import pytest
import torch

import hist_match_ref as href
import vae_encoder_ref as enc_ref
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import makeup_score as ms
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.diffmk.makeups import BaseModel
from oracle import nets, vae

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hist_match_ref.npz'))
CASES = (0, 1, 2)
NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])      # f = 8


def case_terms(k):
    """the 8 terms of golden case k as dense device tensors: term 2 r + d"""
    A = torch.from_numpy(GOLD[f'c{k}_img_a'].astype(np.float32) / np.float32(65535.0))
    B = torch.from_numpy(GOLD[f'c{k}_img_b'].astype(np.float32) / np.float32(65535.0))
    ma, mb = torch.from_numpy(GOLD[f'c{k}_mask_a']), torch.from_numpy(GOLD[f'c{k}_mask_b'])
    dst = torch.stack([A if d == 0 else B for r in range(4) for d in range(2)])
    ref = torch.stack([B if d == 0 else A for r in range(4) for d in range(2)])
    md = torch.stack([ma[r] if d == 0 else mb[r] for r in range(4) for d in range(2)])
    mr = torch.stack([mb[r] if d == 0 else ma[r] for r in range(4) for d in range(2)])
    return dst.to(DEV), ref.to(DEV), md.to(DEV), mr.to(DEV)


def loss64(k, dst, md):
    return np.array([href.loss_f64(dst[t].cpu().numpy(), md[t].cpu().numpy(), GOLD[f'c{k}_matched'][t]) for t in range(8)])


def check_case(k, matched, tables, loss, counts, dst, md, terms=range(8)):
    terms = list(terms)
    ca, cb = GOLD[f'c{k}_count_a'], GOLD[f'c{k}_count_b']
    want_counts = np.array([[ca[t // 2], cb[t // 2]] if t % 2 == 0 else [cb[t // 2], ca[t // 2]] for t in terms])
    assert np.array_equal(tables.cpu().numpy(), GOLD[f'c{k}_tables'][terms])
    assert np.array_equal(matched.cpu().numpy(), GOLD[f'c{k}_matched'][terms].astype(np.float32))
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    l64 = loss64(k, dst, md)[terms]
    rel = np.abs(loss.cpu().numpy().astype(np.float64) - l64) / l64
    print(f'case {k} terms {terms}: loss rel err vs float64 max {rel.max():.3e}')
    assert rel.max() <= 1e-5


# ---- 1. against the reference's recorded results ----------------------------------------------------------------------------
@pytest.mark.parametrize('k', CASES)
def test_region_masks_equal_the_reference(k):
    for side in 'ab':
        seg = torch.from_numpy(GOLD[f'c{k}_seg_{side}'])[None].to(DEV)
        masks, counts = ms.region_masks(seg)
        for r, name in enumerate(ms.REGIONS):
            assert np.array_equal(masks[name][0].cpu().numpy(), GOLD[f'c{k}_mask_{side}'][r]), (k, side, name)
            assert int(counts[name][0]) == int(GOLD[f'c{k}_count_{side}'][r])


@pytest.mark.parametrize('k', CASES)
def test_all_terms_in_one_call_equal_the_reference(k):
    dst, ref, md, mr = case_terms(k)
    matched, tables, loss, counts = ms.histogram_match(dst, ref, md, mr)
    check_case(k, matched, tables, loss, counts, dst, md)


@pytest.mark.parametrize('k', CASES)
def test_single_terms_equal_the_reference_and_the_batched_call_bit_for_bit(k):
    dst, ref, md, mr = case_terms(k)
    mb, tb, lb, cb = ms.histogram_match(dst, ref, md, mr)
    for t in range(8):
        m1, t1, l1, c1 = ms.histogram_match(dst[t:t + 1], ref[t:t + 1], md[t:t + 1], mr[t:t + 1])
        check_case(k, m1, t1, l1, c1, dst, md, terms=[t])
        assert torch.equal(m1[0], mb[t]) and torch.equal(t1[0], tb[t]) and torch.equal(c1[0], cb[t])
        assert l1.view(torch.int32)[0].item() == lb.view(torch.int32)[t].item(), (t, l1.item(), lb[t].item())
    m2, t2, l2, c2 = ms.histogram_match(dst, ref, md, mr)
    assert torch.equal(m2, mb) and torch.equal(t2, tb) and torch.equal(c2, cb) and torch.equal(l2.view(torch.int32), lb.view(torch.int32))


def test_two_cases_in_one_call_through_the_index_table():
    """the index form: images and masks stay where they are, term rows pick them (both 128^2 cases in one call)"""
    parts = [case_terms(k) for k in (0, 1)]
    imgs = torch.cat([p[0][0:2] for p in parts])              # A0, B0, A1, B1
    masks = torch.cat([torch.from_numpy(GOLD[f'c{k}_mask_{s}']) for k in (0, 1) for s in 'ab']).to(DEV)      # [16]: (k, side, region)
    rows = []
    for k in (0, 1):
        for r in range(4):
            a, b, ma, mb = 2 * k, 2 * k + 1, 8 * k + r, 8 * k + 4 + r
            rows += [(a, b, ma, mb), (b, a, mb, ma)]
    index = torch.tensor(rows, dtype=torch.int32).to(DEV)
    matched, tables, loss, counts = ms.histogram_match(imgs, imgs, masks, masks, index=index)
    for i, k in enumerate((0, 1)):
        sl = slice(8 * i, 8 * i + 8)
        check_case(k, matched[sl], tables[sl], loss[sl], counts[sl], parts[i][0], parts[i][2])


# ---- 2. C ABI: unwritten elements, optional outputs, argument errors ----------------------------------------------------------
def test_c_abi_writes_every_element_and_refuses_bad_arguments():
    lib = L()
    dst, ref, md, mr = case_terms(0)
    n, H, W = 8, 128, 128
    scratch = torch.full((int(lib.mkd_hist_match_scratch_bytes(n)),), 0xA5, dtype=torch.uint8, device=DEV)
    matched = torch.full((n, 3, H, W), float('nan'), device=DEV)
    tables = torch.full((n, 3, 256), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((n,), float('nan'), device=DEV)
    counts = torch.full((n, 2), -1, dtype=torch.int32, device=DEV)
    assert lib.mkd_hist_match(P(dst), P(ref), P(md), P(mr), None, n, H, W, P(matched), P(tables), P(loss), P(counts), P(scratch), None) == 0
    sync()
    check_case(0, matched, tables, loss, counts, dst, md)
    # tables only, loss only
    t2 = torch.full_like(tables, 0xFF)
    assert lib.mkd_hist_match(P(dst), P(ref), P(md), P(mr), None, n, H, W, None, P(t2), None, None, P(scratch), None) == 0
    l2 = torch.full_like(loss, float('nan'))
    assert lib.mkd_hist_match(P(dst), P(ref), P(md), P(mr), None, n, H, W, None, None, P(l2), None, P(scratch), None) == 0
    sync()
    assert torch.equal(t2, tables) and torch.equal(l2.view(torch.int32), loss.view(torch.int32))
    assert lib.mkd_hist_match_launches(1, 1) <= 5 and lib.mkd_hist_match_launches(0, 0) == 3
    assert lib.mkd_hist_match_scratch_bytes(0) == 0
    for bad in ((P(dst), P(ref), P(md), P(mr), None, n, H, W, None, None, None, P(counts), P(scratch), None),          # no output
                (P(dst), P(ref), P(md), P(mr), None, 0, H, W, P(matched), None, None, None, P(scratch), None),
                (P(dst), P(ref), P(md), P(mr), None, n, 0, W, P(matched), None, None, None, P(scratch), None),
                (None, P(ref), P(md), P(mr), None, n, H, W, P(matched), None, None, None, P(scratch), None),
                (P(dst), P(ref), P(md), P(mr), None, n, H, W, P(matched), None, None, None, None, None)):
        assert lib.mkd_hist_match(*bad) == -1
    seg = torch.from_numpy(GOLD['c0_seg_a'])[None].to(DEV)
    mk = torch.full((1, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    box = torch.full((1, 4), -7, dtype=torch.int32, device=DEV)
    assert lib.mkd_region_mask_from_labels(P(seg), 1, H, W, 0b1000010, 1 << 4, 10, P(mk), P(cnt), P(box), None) == 0
    sync()
    ys, xs = np.nonzero(GOLD['c0_seg_a'] == 4)
    assert box[0].tolist() == [ys.min(), ys.max(), xs.min(), xs.max()]
    assert np.array_equal(mk[0].cpu().numpy(), GOLD['c0_mask_a'][2]) and int(cnt[0]) == int(GOLD['c0_count_a'][2])
    assert lib.mkd_region_mask_from_labels(P(seg), 1, H, W, 2, 1 << 4, 10, P(mk), P(cnt), None, None) == -1      # a box needs box_out
    assert lib.mkd_region_mask_from_labels(P(seg), 0, H, W, 2, 0, 10, P(mk), P(cnt), None, None) == -1
    assert lib.mkd_region_mask_from_labels(P(seg), 1, H, W, 2, 0, -1, P(mk), P(cnt), None, None) == -1
    assert lib.mkd_region_mask_from_labels(None, 1, H, W, 2, 0, 10, P(mk), P(cnt), None, None) == -1


# ---- 3. build-defined cases against the restatement ---------------------------------------------------------------------------------
def run_against_restatement(dst, ref, md, mr, offset=0):
    """dense terms through the C ABI with every output pre-filled (matched / loss NaN, tables 0xFF, counts -1, scratch 0xA5), so that
    an unwritten element shows, == the restatement; then the Python layer must give the same bits.  offset: the images start that
    many floats into their allocation (a 4-byte aligned base: the scalar-load form of the kernels)."""
    lib = L()
    n, _, H, W = dst.shape
    def place(t):
        buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=DEV)
        v = buf[offset:].view(t.shape)
        v.copy_(t)
        return v
    d, r, mdd, mrd = place(dst), place(ref), md.to(DEV).contiguous(), mr.to(DEV).contiguous()
    scratch = torch.full((int(lib.mkd_hist_match_scratch_bytes(n)),), 0xA5, dtype=torch.uint8, device=DEV)
    matched = torch.full((n, 3, H, W), float('nan'), device=DEV)
    tables = torch.full((n, 3, 256), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.full((n,), float('nan'), device=DEV)
    counts = torch.full((n, 2), -1, dtype=torch.int32, device=DEV)
    assert lib.mkd_hist_match(P(d), P(r), P(mdd), P(mrd), None, n, H, W, P(matched), P(tables), P(loss), P(counts), P(scratch), None) == 0
    sync()
    assert torch.isfinite(matched).all() and torch.isfinite(loss).all()
    for t in range(n):
        m, tab, l, c = href.histogram_match(dst[t].numpy(), ref[t].numpy(), md[t].numpy(), mr[t].numpy())
        assert np.array_equal(tables[t].cpu().numpy(), tab), t
        assert np.array_equal(matched[t].cpu().numpy(), m), t
        assert counts[t].tolist() == list(c), t
        l64 = 0.0 if 0 in c else href.loss_f64(dst[t].numpy(), md[t].numpy(), m)          # an empty side: loss 0 by definition
        assert float(l) == 0.0 if 0 in c else abs(float(l) - l64) <= 1e-5 * l64
        assert abs(float(loss[t]) - l64) <= 1e-5 * l64, (t, float(loss[t]), l64)
    # matched alone and loss alone (the apply kernel without its other output), pre-filled again
    m2 = torch.full_like(matched, float('nan'))
    assert lib.mkd_hist_match(P(d), P(r), P(mdd), P(mrd), None, n, H, W, P(m2), None, None, None, P(scratch), None) == 0
    l2 = torch.full_like(loss, float('nan'))
    assert lib.mkd_hist_match(P(d), P(r), P(mdd), P(mrd), None, n, H, W, None, None, P(l2), None, P(scratch), None) == 0
    sync()
    assert torch.equal(m2, matched) and torch.equal(l2.view(torch.int32), loss.view(torch.int32))
    pm, pt, pl, pc = ms.histogram_match(dst.to(DEV), ref.to(DEV), mdd, mrd)
    assert torch.equal(pm, matched) and torch.equal(pt, tables) and torch.equal(pc, counts)
    assert torch.equal(pl.view(torch.int32), loss.view(torch.int32))          # (offset > 0: the other load form, the same bits)
    return matched, tables, loss, counts


def test_empty_and_full_regions():
    g = torch.Generator().manual_seed(81)
    H, W = 64, 64
    dst, ref = torch.rand(4, 3, H, W, generator=g) ** 2, 0.3 + 0.6 * torch.rand(4, 3, H, W, generator=g)
    some = (torch.rand(4, H, W, generator=g) > 0.6).to(torch.uint8)
    md, mr = some.clone(), some.flip(0).clone()
    md[0] = 0                       # empty dst region
    mr[1] = 0                       # empty ref region
    md[2] = 1; mr[2] = 1            # full masks
    matched, tables, loss, counts = run_against_restatement(dst, ref, md, mr)
    ident = torch.arange(256, dtype=torch.uint8, device=DEV).expand(3, 256)
    for t in (0, 1):
        assert torch.equal(tables[t], ident) and float(loss[t]) == 0.0 and not matched[t].any()
    assert counts[0, 0] == 0 and counts[1, 1] == 0 and counts[2].tolist() == [H * W, H * W]
    assert float(loss[2]) > 0 and float(loss[3]) > 0


@pytest.mark.parametrize('hw', [(48, 80), (37, 53)])
def test_non_square_images(hw):
    """(37, 53): H W is odd, the scalar-load form of the kernels"""
    g = torch.Generator().manual_seed(82)
    H, W = hw
    dst, ref = torch.rand(3, 3, H, W, generator=g), torch.rand(3, 3, H, W, generator=g) ** 3
    md, mr = (torch.rand(3, H, W, generator=g) > 0.5).to(torch.uint8), (torch.rand(3, H, W, generator=g) > 0.3).to(torch.uint8)
    md[1] = 0                       # an empty dst region in these forms too
    run_against_restatement(dst, ref, md, mr)
    run_against_restatement(dst, ref, md, mr, offset=1)          # images 4-byte aligned only: scalar loads whatever H W is


def test_values_outside_the_unit_interval_and_exactly_one():
    g = torch.Generator().manual_seed(83)
    H, W = 32, 64
    dst = torch.rand(2, 3, H, W, generator=g) * 1.6 - 0.3              # below 0 and above 1
    ref = torch.rand(2, 3, H, W, generator=g)
    dst[0, :, :4] = 1.0
    ref[1, :, 5:9] = 1.0
    dst[1, 0, 10] = 0.0
    md, mr = torch.ones(2, H, W, dtype=torch.uint8), (torch.rand(2, H, W, generator=g) > 0.2).to(torch.uint8)
    matched, *_ = run_against_restatement(dst, ref, md, mr)
    assert float(matched.max()) <= 255.0


def test_eye_box_is_clipped_at_the_border_and_absent_labels_give_empty_regions():
    seg = np.ones((2, 40, 56), np.uint8)
    seg[0, 2:6, 1:9] = 4               # left eye 2 px from the top, 1 px from the left: the grown box leaves the image
    seg[0, 30:38, 50:56] = 5           # right eye touching the right border
    seg[0, 20:24, 20:30] = 7
    seg[1, 10:14, 10:20] = 4           # pair 1: no right eye, no lips
    lib, lab = L(), torch.from_numpy(seg).to(DEV)
    sets = {'lip': (href.LIP, ()), 'skin': (href.SKIN, ()), 'eye_left': (href.FACE, href.EYE_LEFT), 'eye_right': (href.FACE, href.EYE_RIGHT)}
    bits = lambda cs: sum(1 << c for c in cs)
    want = [href.region_masks(seg[b]) for b in range(2)]
    for name, (cls, box_cls) in sets.items():          # the C ABI with pre-filled outputs: an unwritten element shows
        mk = torch.full((2, 40, 56), 0xFF, dtype=torch.uint8, device=DEV)
        cnt = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        box = torch.full((2, 4), -1, dtype=torch.int32, device=DEV)
        assert lib.mkd_region_mask_from_labels(P(lab), 2, 40, 56, bits(cls), bits(box_cls), 10, P(mk), P(cnt), P(box) if box_cls else None, None) == 0
        sync()
        for b in range(2):
            assert np.array_equal(mk[b].cpu().numpy(), want[b][name]), (b, name)
            assert int(cnt[b]) == int(want[b][name].sum()), (b, name)
        if name == 'eye_left':
            assert box.tolist() == [[2, 5, 1, 8], [10, 13, 10, 19]]
        if name == 'eye_right':
            assert box.tolist() == [[30, 37, 50, 55], [2 ** 31 - 1, -1, 2 ** 31 - 1, -1]]
    masks, counts = ms.region_masks(lab)
    for b in range(2):
        for name in ms.REGIONS:
            assert np.array_equal(masks[name][b].cpu().numpy(), want[b][name]), (b, name)
            assert int(counts[name][b]) == int(want[b][name].sum())
    assert int(counts['eye_right'][1]) == 0 and int(counts['lip'][1]) == 0
    assert int(counts['eye_left'][0]) == 16 * 19 - 4 * 8          # rows 0..15, cols 0..18 of face labels minus the eye itself
    _, _, box = ms.region_mask(lab, (1, 6), (5,))
    assert box[0].tolist() == [30, 37, 50, 55] and box[1].tolist() == [2 ** 31 - 1, -1, 2 ** 31 - 1, -1]


# ---- 4. the eight terms of a batch ------------------------------------------------------------------------------------------------------
def face_seg(res, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:res, 0:res].astype(np.float64)
    cy, cx = res * (0.5 + 0.04 * g.standard_normal()), res * (0.5 + 0.04 * g.standard_normal())
    ell = lambda dy, dx, ry, rx: ((yy - cy - dy * res) / (ry * res)) ** 2 + ((xx - cx - dx * res) / (rx * res)) ** 2 <= 1.0
    seg = np.zeros((res, res), np.uint8)
    seg[ell(0.3, 0, 0.15, 0.15)] = 13
    seg[ell(0, 0, 0.34, 0.27)] = 1
    seg[ell(0.02, 0, 0.07, 0.03)] = 6
    seg[ell(-0.09, -0.11, 0.03, 0.05)] = 4
    seg[ell(-0.09, 0.11, 0.03, 0.05)] = 5
    seg[ell(0.18, 0, 0.04, 0.09)] = 7
    seg[ell(0.18, 0, 0.04, 0.09) & (yy > cy + 0.18 * res)] = 9
    return seg


def test_makeup_hist_terms_of_a_batch_equal_the_restatement_pair_by_pair():
    g = torch.Generator().manual_seed(84)
    B, res = 3, 96
    SR, RS, S, R = (torch.rand(B, 3, res, res, generator=g) ** p for p in (2.0, 0.5, 1.0, 1.5))
    src_seg = np.stack([face_seg(res, 100 + b) for b in range(B)])
    ref_seg = np.stack([face_seg(res, 200 + b) for b in range(B)])
    lam = dict(lip=1.0, skin_1=0.1, skin_2=0.2, eye=0.5)
    out = ms.makeup_hist_terms(SR.to(DEV), RS.to(DEV), S.to(DEV), R.to(DEV), torch.from_numpy(src_seg).to(DEV), torch.from_numpy(ref_seg).to(DEV), lam)
    w = dict(sr_lip=1.0, rs_lip=1.0, sr_skin=0.1, rs_skin=0.2)
    for b in range(B):
        want = href.makeup_terms(SR[b].numpy(), RS[b].numpy(), S[b].numpy(), R[b].numpy(), src_seg[b], ref_seg[b])
        for name in ms.TERMS:
            assert want[name] > 0
            assert abs(float(out[name][b]) - w.get(name, 0.5) * float(want[name])) <= 2e-5 * float(want[name]), (b, name)
        lm = href.loss_makeup(want, 1.0, 0.1, 0.2, 0.5)
        assert abs(float(out['loss_makeup'][b]) - lm) <= 2e-5 * lm
    assert tuple(out['counts'].shape) == (8, B, 2) and int(out['counts'].min()) > 0
    # one pair alone == its row of the batch, bit for bit
    one = ms.makeup_hist_terms(SR[1:2].to(DEV), RS[1:2].to(DEV), S[1:2].to(DEV), R[1:2].to(DEV), torch.from_numpy(src_seg[1:2]).to(DEV),
                               torch.from_numpy(ref_seg[1:2]).to(DEV), lam)
    for name in ms.TERMS + ('loss_makeup',):
        assert one[name].view(torch.int32)[0].item() == out[name].view(torch.int32)[1].item(), name


# ---- 5. the model surface -----------------------------------------------------------------------------------------------------------------
def model_sd(hint_channels, seed):
    ocfg = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                          hint_widths=tuple(HINT_WIDTHS), hint_channels=hint_channels)
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    return {**nets.init_state_dict(ocfg, seed=seed), **vae.init_state_dict(vcfg, seed=seed + 1), **enc_ref.init_state_dict(vcfg, seed=seed + 2)}


def test_validation_losses_equal_the_restatement_on_the_generated_images():
    m = BaseModel(control_stage_config={'params': dict(NET, hint_channels=3, hint_widths=HINT_WIDTHS)},
                  unet_config={'params': dict(NET, out_channels=4)},
                  first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True, iter_finetune=4,
                  weight_loss_makeup=0.7, weight_loss_background=2.0, weight_loss_idt=0.3, weight_loss_cycle=0.0,
                  lambda_his_lip=1.0, lambda_his_skin_1=0.1, lambda_his_skin_2=0.1, lambda_his_eye=0.5)
    m.load_state_dict(model_sd(3, 41))
    m.cuda(0)
    g = torch.Generator().manual_seed(85)
    B, res = 2, 64
    src_seg = np.stack([face_seg(res, 300 + b) for b in range(B)])
    ref_seg = np.stack([face_seg(res, 400 + b) for b in range(B)])
    batch = {'src_img': torch.rand(B, 3, res, res, generator=g), 'ref_img': torch.rand(B, 3, res, res, generator=g),
             'txt_emb': torch.randn(B, 77, 64, generator=g), 'src_inv': torch.randn(B, 4, 8, 8, generator=g),
             'ref_inv': torch.randn(B, 4, 8, 8, generator=g), 'src_msk': torch.from_numpy(src_seg), 'ref_msk': torch.from_numpy(ref_seg)}
    loss, ld, im = m.validation_losses(batch, return_images=True)
    assert set(ld) == {'val/loss_background', 'val/loss_makeup', 'val/loss_idt'} | {'val/his_' + t for t in ms.TERMS}
    SR, RS = im['fake_SR'].cpu().numpy(), im['fake_RS'].cpu().numpy()
    S, R = batch['src_img'].numpy(), batch['ref_img'].numpy()
    terms = [href.makeup_terms(SR[b], RS[b], S[b], R[b], src_seg[b], ref_seg[b]) for b in range(B)]
    lam = dict(sr_lip=1.0, rs_lip=1.0, sr_skin=0.1, rs_skin=0.1)
    for name in ms.TERMS:
        want = np.mean([lam.get(name, 0.5) * float(t[name]) for t in terms])
        assert abs(float(ld['val/his_' + name]) - want) <= 2e-5 * abs(want) + 1e-12, name
    mk = np.mean([href.loss_makeup(t, 1.0, 0.1, 0.1, 0.5) for t in terms])
    assert abs(float(ld['val/loss_makeup']) - mk) <= 2e-5 * mk
    bg_s = (np.abs(SR - S) * np.isin(src_seg, (0, 10, 13))[:, None]).mean((1, 2, 3)).mean()
    bg_r = (np.abs(RS - R) * np.isin(ref_seg, (0, 10, 13))[:, None]).mean((1, 2, 3)).mean()
    assert abs(float(ld['val/loss_background']) - 0.5 * (bg_s + bg_r)) <= 1e-5
    idt = 0.5 * (np.abs(im['fake_SS'].cpu().numpy() - S).mean() + np.abs(im['fake_RR'].cpu().numpy() - R).mean())
    assert abs(float(ld['val/loss_idt']) - idt) <= 1e-5
    total = 2.0 * float(ld['val/loss_background']) + 0.7 * float(ld['val/loss_makeup']) + 0.3 * float(ld['val/loss_idt'])
    assert abs(float(loss) - total) <= 1e-5 * abs(total)
    with pytest.raises(NotImplementedError):
        m.shared_step(batch)
    m.engine.close()


def test_log_results_carries_makeup_hist_and_is_unchanged_without_it():
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, ddim_steps=4, unconditional_guidance_scale=9)
    m.load_state_dict(model_sd(6, 51))
    m.cuda(0)
    g = torch.Generator().manual_seed(86)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=g)
    m.save_images = False
    B, res = 2, 64
    src_seg = np.stack([face_seg(res, 500 + b) for b in range(B)])
    ref_seg = np.stack([face_seg(res, 600 + b) for b in range(B)])
    batch = {'src_img': torch.rand(B, 3, res, res, generator=g), 'ref_img': torch.rand(B, 3, res, res, generator=g),
             'txt_emb': torch.randn(B, 77, 64, generator=g), 'nonmakeup_seg': torch.from_numpy(src_seg), 'makeup_seg': torch.from_numpy(ref_seg)}
    x_T = torch.randn(B, 4, 8, 8, generator=g).to(DEV)
    assert m.makeup_score is False
    base = m.log_results(batch, 0, x_T=x_T)
    assert not any(k.startswith('makeup_hist') for k in base)
    m.makeup_score = True
    log = m.log_results(batch, 0, x_T=x_T)
    with pytest.raises(KeyError):
        m.log_results({k: v for k, v in batch.items() if k != 'makeup_seg'}, 0, x_T=x_T)
    extra = {'makeup_hist': 'samples', 'makeup_hist_cfg_scale_9.00': 'samples_cfg_scale_9.00'}
    assert set(log) == set(base) | set(extra)
    for k in base:
        assert torch.equal(log[k], base[k]), k
    R = batch['ref_img'].numpy()
    for k, img_key in extra.items():
        assert tuple(log[k].shape) == (B, 4)
        img = ((log[img_key].float() + 1.0) / 2.0).clamp(0, 1).cpu().numpy()
        for b in range(B):
            ms_, mr_ = href.region_masks(src_seg[b]), href.region_masks(ref_seg[b])
            for r, name in enumerate(ms.REGIONS):
                want = float(href.histogram_match(img[b], R[b], ms_[name], mr_[name])[2])
                assert want > 0 and abs(float(log[k][b, r]) - want) <= 2e-5 * want, (k, b, name)
    out = m.test_step(batch, 0, x_T=x_T)               # the scores are not clamped like images
    assert torch.equal(out['makeup_hist'], log['makeup_hist'].cpu())
    m.engine.close()
