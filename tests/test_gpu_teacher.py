"""-m gpu: the histogram-matching teacher on the device.  mkd_pgt_compose is held BIT FOR BIT to the numpy restatement
(tests/teacher_ref.py: region ids, window counts, the double expression, one rounding) on every path of the kernel -- feather 0 (no
halo) and > 0, the 16-byte and the scalar form, tiles smaller than, equal to and ragged against 16 x 16 -- and
teacher.pseudo_ground_truth to masks -> hist_match_ref tables -> the restatement."""
import numpy as np
import pytest
import torch

import teacher_ref as tr
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import makeup_score as ms
from makeupdiffuse_amd import teacher

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (16, 16), (17, 33), (40, 24)]
PAD = 64          # canary floats on both sides of the output


def random_case(n, H, W, seed):
    rng = np.random.RandomState(seed)
    src = rng.uniform(-0.1, 1.1, (n, 3, H, W)).astype(np.float32)
    src[:, :, 0, 0] = (rng.randint(0, 256, (n, 3)) / 255).astype(np.float32)
    src[:, :, -1, -1] = np.float32(-0.0)          # a negative zero comes out as +0, under a region or not
    masks = (rng.rand(4, n, H, W) < 0.35).astype(np.uint8) * rng.randint(1, 256, (4, n, H, W)).astype(np.uint8)
    tables = rng.randint(0, 256, (4, n, 3, 256)).astype(np.uint8)
    return src, masks, tables


def mixed_strengths(n, seed):
    a = np.random.RandomState(seed).rand(n, 4).astype(np.float32)
    a[0, 0], a[0, 1], a[-1, 2], a[-1, 3] = 0.0, 1.0, 1.0, 0.0
    return a


def run(src, masks, tables, strengths, F, src_off=0, out_off=0, mask_off=0, tab_off=0):
    """mkd_pgt_compose with the operands `*_off` elements past a 256-byte aligned base, the output between canaries -> numpy"""
    def put(a, off, dtype):
        buf = torch.zeros(a.size + off + 64, dtype=dtype, device=DEV)
        view = buf[off:off + a.size]
        view.copy_(torch.from_numpy(a.reshape(-1)))
        return buf, view
    n, _, H, W = src.shape
    _s, s = put(src, src_off, torch.float32)
    _m, m = put(masks, mask_off, torch.uint8)
    _t, t = put(tables, tab_off, torch.uint8)
    a = None if strengths is None else torch.from_numpy(strengths).to(DEV)
    obuf = torch.full((PAD + out_off + src.size + PAD,), -7.0, dtype=torch.float32, device=DEV)
    o = obuf[PAD + out_off:PAD + out_off + src.size]
    assert s.data_ptr() % 16 == (4 * src_off) % 16 and o.data_ptr() % 16 == (4 * out_off) % 16
    rc = L().mkd_pgt_compose(P(s), P(m), P(t), P(a), n, H, W, F, P(o), None)
    assert rc == 0, L().mkd_last_error()
    sync()
    got = obuf.cpu().numpy()
    assert (got[:PAD + out_off] == -7.0).all() and (got[PAD + out_off + src.size:] == -7.0).all(), 'wrote outside the output'
    return got[PAD + out_off:PAD + out_off + src.size].reshape(src.shape)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('F', [0, 1, 3, 8])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_compose_equals_the_restatement_bit_for_bit(shape, n, F):
    H, W = shape
    src, masks, tables = random_case(n, H, W, 100 * H + 10 * n + F)
    a = None if n == 1 else mixed_strengths(n, F)          # NULL strengths, and mixed values with exact 0 and 1
    got = run(src, masks, tables, a, F)
    want = tr.compose(src, masks, tables, a, F)
    assert same_bits(got, want), f'{(got != want).sum()} of {got.size} values differ, max {np.abs(got - want).max()}'


def shaped_masks(H, W):
    """name -> masks [4, 1, H, W]"""
    z = lambda: np.zeros((4, 1, H, W), dtype=np.uint8)
    out = {}
    m = z(); m[1, 0, 0, :] = m[1, 0, -1, :] = m[1, 0, :, 0] = m[1, 0, :, -1] = 1; m[0, 0, H // 2, 1:W - 1] = 1
    out['a region on all four borders'] = m
    m = z(); m[0, 0, :, W // 2] = 1; m[2, 0, H // 3, :] = 1; m[3, 0, 0, 0] = 1
    out['regions one pixel wide'] = m
    m = z(); m[:, 0, 2:H - 1, 1:W - 2] = 1
    out['all four regions overlapping'] = m
    m = z(); m[3] = 1
    out['an empty region and an all-ones region'] = m
    return out


@pytest.mark.parametrize('F', [0, 3, 8])
@pytest.mark.parametrize('shape', [(17, 33), (40, 24)])
def test_compose_on_shaped_regions(shape, F):
    H, W = shape
    src, _, tables = random_case(1, H, W, H + F)
    for name, masks in shaped_masks(H, W).items():
        got = run(src, masks, tables, None, F)
        assert same_bits(got, tr.compose(src, masks, tables, None, F)), name
    # the consequences the header states: an identity table and a = 0 leave float(v / 255); k / 255 values come back bit for bit
    k = np.random.RandomState(3).randint(0, 256, src.shape)
    exact = (k / 255).astype(np.float32)
    ident = np.tile(np.arange(256, dtype=np.uint8), (4, 1, 3, 1))
    masks = shaped_masks(H, W)['all four regions overlapping']
    assert same_bits(run(exact, masks, ident, None, F), exact)
    assert same_bits(run(exact, masks, tables, np.zeros((1, 4), np.float32), F), exact)


@pytest.mark.parametrize('F', [0, 3])
@pytest.mark.parametrize('shape', [(16, 16), (40, 24)])
def test_unaligned_operands_take_the_scalar_form_with_the_same_bits(shape, F):
    H, W = shape
    src, masks, tables = random_case(3, H, W, 7 + F)
    a = mixed_strengths(3, 1)
    want = tr.compose(src, masks, tables, a, F)
    assert same_bits(run(src, masks, tables, a, F), want)                                   # 16-byte form
    assert same_bits(run(src, masks, tables, a, F, src_off=1), want)                        # src 4 bytes past 16-byte alignment
    assert same_bits(run(src, masks, tables, a, F, out_off=1), want)
    assert same_bits(run(src, masks, tables, a, F, src_off=1, out_off=1), want)
    assert same_bits(run(src, masks, tables, a, F, mask_off=1, tab_off=3), want)            # byte-aligned masks and tables


def test_refusals_leave_the_output_untouched():
    lib = L()
    src, masks, tables = random_case(1, 8, 8, 0)
    s, m, t = (torch.from_numpy(x).to(DEV) for x in (src, masks, tables))
    big = torch.zeros(2 * src.size + 1, dtype=torch.float32, device=DEV)
    out = torch.full(src.shape, -7.0, dtype=torch.float32, device=DEV)
    ok = dict(src=s, masks=m, tables=t, a=None, n=1, H=8, W=8, F=2, out=out)
    bad = [dict(src=None), dict(masks=None), dict(tables=None), dict(n=0), dict(n=65536), dict(H=0), dict(W=0), dict(W=-8), dict(H=4097, W=4096),
           dict(F=-1), dict(F=9)]
    for kw in bad:
        q = {**ok, **kw}
        assert lib.mkd_pgt_compose(P(q['src']), P(q['masks']), P(q['tables']), P(q['a']), q['n'], q['H'], q['W'], q['F'], P(q['out']), None) == -1, kw
        assert lib.mkd_last_error()
    assert lib.mkd_pgt_compose(P(s), P(m), P(t), None, 1, 8, 8, 2, None, None) == -1
    # out may not alias or overlap src
    big[:src.size].copy_(s.reshape(-1))
    before = big.clone()
    for off in (0, 1, src.size - 1):
        assert lib.mkd_pgt_compose(P(big), P(m), P(t), None, 1, 8, 8, 2, P(big[off:]), None) == -1, off
    sync()
    assert torch.equal(big, before) and bool((out == -7.0).all())
    assert lib.mkd_pgt_compose(P(big), P(m), P(t), None, 1, 8, 8, 2, P(big[src.size:]), None) == 0          # adjacent is fine
    sync()
    assert same_bits(big[src.size:2 * src.size].cpu().numpy().reshape(src.shape), tr.compose(src, masks, tables, None, 2))
    assert lib.mkd_pgt_launches() == 1


@pytest.fixture(scope='module')
def pairs():
    src, ref, ss, rs = tr.synthetic_pairs()
    dev = tuple(torch.from_numpy(x).to(DEV) for x in (src, ref, ss, rs))
    return (src, ref, ss, rs), dev


@pytest.mark.parametrize('feather,strengths', [(2, None), (0, None), (3, {'lip': 0.5, 'eye': [1.0, 0.0, 0.25], 'skin': 1.0})])
def test_pseudo_ground_truth_end_to_end(pairs, feather, strengths):
    (src, ref, ss, rs), dev = pairs
    x_p, tables, counts = teacher.pseudo_ground_truth(*dev, strengths=strengths, feather=feather)
    rows = teacher.strength_rows(strengths, 3)
    want, wtab, wcnt, _ = tr.pseudo_ground_truth(src, ref, ss, rs, None if rows is None else rows.numpy(), feather)
    assert tuple(tables.shape) == (4, 3, 3, 256) and tuple(counts.shape) == (4, 3, 2) and counts.dtype == torch.int32
    assert np.array_equal(tables.cpu().numpy(), wtab)
    assert np.array_equal(counts.cpu().numpy(), wcnt)
    assert x_p.dtype == torch.float32 and same_bits(x_p.cpu().numpy(), want)
    assert teacher.launches() == 16
    with pytest.raises(ValueError):
        teacher.pseudo_ground_truth(*dev, strengths={'lip': 1.5})
    with pytest.raises(ValueError):
        teacher.pseudo_ground_truth(*dev, feather=9)
    with pytest.raises(ValueError):
        teacher.pseudo_ground_truth(dev[0], dev[1][:2], dev[2], dev[3])


def test_teacher_lowers_the_score_on_the_synthetic_pairs(pairs):
    """transfer_score(x_p) < transfer_score(source) in every region (all sides are non-empty on these pairs; test_teacher_host.py shows
    the same on the restatement alone)"""
    _, (s, r, ss, rs) = pairs
    base = ms.transfer_score(s, r, ss, rs).cpu().numpy()
    for F in (0, 2):
        x_p, _, counts = teacher.pseudo_ground_truth(s, r, ss, rs, feather=F)
        assert int(counts.min()) > 0
        score = ms.transfer_score(x_p, r, ss, rs).cpu().numpy()
        print(f'feather {F}: source {base.tolist()} teacher {score.tolist()}')
        assert (score < base).all()
