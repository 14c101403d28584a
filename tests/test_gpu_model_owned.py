"""-m gpu: TestDiffuseModel.transfer_photos(max_faces=..., own_pixels=True) on the small model and the stub parser of
tests/test_gpu_model_faces.py.  A 128 x 128 photo shows two faces so close that the large face's grown box covers the small one, and a
second photo shows none.  Every test first asserts what makes it mean something: the box does cover the small face, and the plain
group-photo call does repaint it.  With own_pixels the call is, byte for byte, the chain of the calls with weights; where one face
owns a whole neighbourhood the bytes are those of pasting that face alone; a face beyond max_faces keeps the photo's bytes."""
import numpy as np
import pytest
import torch

import owner_ref as orf
from gpu_util import DEV
from makeupdiffuse_amd import components
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import photo
from test_gpu_model_faces import EMPTY, PS, S, StubParser, blobs, m, model, sample_chunk  # noqa: F401  (fixtures: an instance for this module)

pytestmark = pytest.mark.gpu

LARGE, SMALL = (8, 27, 8, 27), (12, 23, 30, 37)          # (row min, row max, col min, col max) in the 64 x 64 parsed map: two columns apart
SRC_MAPS = torch.stack([blobs(LARGE + (1,), SMALL + (1,)), EMPTY])
REF_MAPS = torch.stack([blobs((10, 50, 12, 48, 1)), blobs((20, 40, 20, 44, 6))])
SRC_SIZES, REF_SIZES = ((128, 128), (80, 100)), ((70, 64), (90, 90))
FEATHER, OWN = 3, 2
_cache = {}


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(417)
    rand = lambda hw: torch.randint(0, 256, (hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    return dict(src=[rand(s) for s in SRC_SIZES], ref=[rand(s) for s in REF_SIZES], batch={'txt_emb': torch.randn(2, 77, 64, generator=g)},
                x_T=torch.randn(2, 4, 8, 8, generator=g))


def photo_mask(box, H, W, erode=0):
    """the photo pixels that map into a box of the parsed map shrunk by ``erode`` parse pixels per side"""
    r0, r1, c0, c1 = box
    py, px = np.arange(H) * PS // H, np.arange(W) * PS // W
    return np.outer((py >= r0 + erode) & (py <= r1 - erode), (px >= c0 + erode) & (px <= c1 - erode))


def setting(m, d):
    """the faces, the owner map and the two decoded samples (computed once), and the two facts every test stands on"""
    if _cache:
        return _cache
    src = [p.to(DEV) for p in d['src']]
    faces, owner = fp.find_faces(StubParser(SRC_MAPS), src, max_faces=2, parse_size=PS, return_owner=True)
    ref_boxes = [f[0] for f in fp.find_faces(StubParser(REF_MAPS), [p.to(DEV) for p in d['ref']], max_faces=1, parse_size=PS)]
    assert [len(f) for f in faces] == [2, 0] and tuple(owner.shape) == (2, PS, PS) and owner.dtype == torch.uint8
    assert faces == fp.find_faces(StubParser(SRC_MAPS), src, max_faces=2, parse_size=PS)
    H, W = SRC_SIZES[0]
    (lx, ly, lw, lh), (sx, sy, sw, sh) = faces[0]
    small_in, large_in = photo_mask(SMALL, H, W, OWN + 1), photo_mask(LARGE, H, W, OWN + 1)
    in_large_box, in_small_box = np.zeros((H, W), bool), np.zeros((H, W), bool)
    in_large_box[ly:ly + lh, lx:lx + lw] = True
    in_small_box[sy:sy + sh, sx:sx + sw] = True
    assert small_in.any() and in_large_box[photo_mask(SMALL, H, W)].all(), 'the large face\'s box must cover the small face'
    assert (large_in & in_small_box).any(), 'the small face\'s box must reach into the large face'
    m.reset_conditioning_cache()
    img, s01 = sample_chunk(m, [src[0], src[0]], faces[0], [d['ref'][0].to(DEV)] * 2, [ref_boxes[0]] * 2, d['batch']['txt_emb'][[0, 0]], d['x_T'])
    alone = []
    for k in range(2):                                   # each face pasted ALONE into the photo, the plain paste
        one = src[0].clone()
        photo.paste_photos([one], [faces[0][k]], img[k:k + 1], s01[k:k + 1], FEATHER)
        alone.append(one.cpu().numpy())
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    m.reset_conditioning_cache()
    plain = m.transfer_photos(d['src'], d['ref'], feather=FEATHER, x_T=d['x_T'], size=S, batch=d['batch'], max_faces=2)
    plain0 = plain[0].cpu().numpy()
    assert (plain0[small_in] != alone[1][small_in]).any(), 'the plain path must repaint the small face from the large face\'s crop'
    # the weights in photo pixels: one face owns these regions outright
    o = owner[0].cpu().numpy()
    w = [orf.weight_at_photo(orf.weights(o, k, OWN), H, W) for k in range(2)]
    assert (w[1][small_in] == 1).all() and (w[0][small_in] == 0).all() and (w[0][large_in] == 1).all() and (w[1][large_in] == 0).all()
    _cache.update(src=src, faces=faces, owner=owner, ref_boxes=ref_boxes, img=img, s01=s01, alone=alone, plain=plain, small_in=small_in,
                  large_in=large_in, in_large_box=in_large_box)
    return _cache


def owned(m, d, **kw):
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    m.reset_conditioning_cache()
    return m.transfer_photos(d['src'], d['ref'], feather=FEATHER, size=S, batch=d['batch'], own_pixels=True, own_feather=OWN, **kw)


def test_owned_paste_is_the_chain_of_the_calls_with_weights(m, data):
    c = setting(m, data)
    got, told = owned(m, data, x_T=data['x_T'], max_faces=2, return_faces=True)
    assert told == c['faces'] and m.face_parser.n == 2                                   # still one parse per side
    want = c['src'][0].clone()
    for k in range(2):
        weights = components.owner_weights(c['owner'], [(0, k)], OWN)
        photo.paste_photos([want], [c['faces'][0][k]], c['img'][k:k + 1], c['s01'][k:k + 1], FEATHER, weights=weights)
    assert got[0].dtype == torch.uint8 and got[0].device.type == 'cuda'
    g, w = got[0].cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(g, w), f'{int((g != w).sum())} bytes differ from the chain of the calls'
    assert not np.array_equal(g, c['plain'][0].cpu().numpy())


def test_each_face_keeps_its_own_pixels(m, data):
    c = setting(m, data)
    g = owned(m, data, x_T=data['x_T'], max_faces=2)[0].cpu().numpy()
    p = data['src'][0].numpy()
    for k, region in ((1, c['small_in']), (0, c['large_in'])):
        assert np.array_equal(g[region], c['alone'][k][region]), f'face {k}: its own pixels carry another face\'s paste'
        assert (g[region] != p[region]).mean() > 0.3                                     # and it was made up


def test_a_face_beyond_max_faces_keeps_the_photos_bytes(m, data):
    c = setting(m, data)
    p = data['src'][0].numpy()
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    m.reset_conditioning_cache()
    plain = m.transfer_photos(data['src'], data['ref'], feather=FEATHER, x_T=data['x_T'][:1], size=S, batch=data['batch'], max_faces=1)[0].cpu().numpy()
    assert (plain[c['small_in']] != p[c['small_in']]).any()                              # today its neighbour repaints it
    got, told = owned(m, data, x_T=data['x_T'][:1], max_faces=1, return_faces=True)
    g = got[0].cpu().numpy()
    assert told == [c['faces'][0][:1], []]
    assert np.array_equal(g[c['small_in']], p[c['small_in']])
    assert (g[c['large_in']] != p[c['large_in']]).mean() > 0.3 and np.array_equal(g[~c['in_large_box']], p[~c['in_large_box']])


def test_own_pixels_false_is_the_call_without_the_argument(m, data):
    c = setting(m, data)
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    m.reset_conditioning_cache()
    got = m.transfer_photos(data['src'], data['ref'], feather=FEATHER, x_T=data['x_T'], size=S, batch=data['batch'], max_faces=2, own_pixels=False)
    assert all(torch.equal(g, w) for g, w in zip(got, c['plain']))


def test_a_faceless_photo_comes_back_unchanged(m, data):
    setting(m, data)
    got = owned(m, data, x_T=data['x_T'], max_faces=2)
    assert torch.equal(got[1].cpu(), data['src'][1]) and not torch.equal(got[0].cpu(), data['src'][0])
    m.face_parser = StubParser(torch.stack([EMPTY, EMPTY]), REF_MAPS)                    # N = 0: nothing is sampled, nothing pasted
    m.reset_conditioning_cache()
    got, told = m.transfer_photos(data['src'], data['ref'], size=S, batch=data['batch'], max_faces=2, own_pixels=True, return_faces=True)
    assert told == [[], []] and all(torch.equal(g.cpu(), p) for g, p in zip(got, data['src']))
