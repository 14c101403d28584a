"""-m gpu: TestDiffuseModel.transfer_photos(max_faces=...) on the small model of tests/test_gpu_model_photo.py at S = 64.  A stub parser
returns fixed label maps, so the faces are known: a 120 x 90 photo with three blobs (two of them with overlapping grown boxes) and a
64 x 64 photo with one.  The group-photo call must be, byte for byte, find_faces -> crop_resize -> the model's own sampling and decode
in the same chunks -> paste_photos rank by rank."""
import numpy as np
import pytest
import torch

from gpu_util import DEV
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import photo
from test_gpu_model_photo import S, model  # noqa: F401  (the module-scoped small model; this module gets an instance of its own)

pytestmark = pytest.mark.gpu

PS = 64                                    # parse size of the stub's label maps
SRC_SIZES, REF_SIZES = ((120, 90), (64, 64)), ((70, 64), (80, 100))


class StubParser:
    """duck-typed face parser: parse() hands out the label maps of ``seq`` in turn (source photos first, then the references)"""

    def __init__(self, *seq):
        self.seq, self.n = [s.to(DEV) for s in seq], 0

    def parse(self, img01, out_size=None, lut=None, return_logits=False):
        maps = self.seq[self.n % len(self.seq)]
        self.n += 1
        assert out_size is None and tuple(img01.shape) == (maps.shape[0], 3, PS, PS)
        return maps


def blobs(*boxes):
    m = torch.zeros(PS, PS, dtype=torch.uint8)
    for r0, r1, c0, c1, label in boxes:
        m[r0:r1 + 1, c0:c1 + 1] = label
    return m


# photo 0: areas 144, 64 (one empty column away from nothing: six columns right of the first), 100 far away; photo 1: one blob
SRC_MAPS = torch.stack([blobs((8, 19, 8, 19, 1), (12, 19, 26, 33, 7), (44, 53, 40, 49, 1)), blobs((20, 45, 18, 44, 1), (30, 33, 25, 35, 9))])
REF_MAPS = torch.stack([blobs((5, 10, 5, 10, 1), (20, 50, 20, 50, 1)), blobs((10, 40, 30, 60, 6))])          # reference 0: the larger face counts
EMPTY = torch.zeros(PS, PS, dtype=torch.uint8)


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(91)
    rand = lambda hw: torch.randint(0, 256, (hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    return dict(src=[rand(s) for s in SRC_SIZES], ref=[rand(s) for s in REF_SIZES], batch={'txt_emb': torch.randn(2, 77, 64, generator=g)},
                x_T=torch.randn(4, 4, 8, 8, generator=g))


@pytest.fixture()
def m(model):  # noqa: F811
    model.parse_size = PS
    model.reset_conditioning_cache()
    yield model
    model.face_parser, model.parse_size = None, 512


def faces_of(maps, photos, K):
    return fp.find_faces(StubParser(maps), [p.to(DEV) for p in photos], max_faces=K, parse_size=PS)


def sample_chunk(m, src_photos, boxes, ref_photos, ref_boxes, ctx, x_T):
    """the single pass transfer_photos runs for one batch, from the existing calls"""
    n = len(boxes)
    src, ref = photo.crop_resize(src_photos, boxes, S).img01, photo.crop_resize(ref_photos, ref_boxes, S).img01
    cond = {'c_concat': [torch.cat((src, ref), 1)], 'c_crossattn': [ctx.to(DEV)]}
    extra = dict(x_T=x_T.to(DEV), unconditional_guidance_scale=float(m.unconditional_guidance_scale),
                 unconditional_conditioning={'c_concat': cond['c_concat'], 'c_crossattn': [m.get_unconditional_conditioning(n)]})
    lat, _ = m.sample_log(cond=cond, batch_size=n, ddim=True, ddim_steps=m.ddim_steps, eta=m.ddim_eta, **extra)
    return m.decode_first_stage(lat), src


def by_hand(m, d, faces, ref_boxes, face_batch, feather):
    src, ref = [p.to(DEV) for p in d['src']], [p.to(DEV) for p in d['ref']]
    items = [(i, k) for i, f in enumerate(faces) for k in range(len(f))]
    imgs, srcs = [], []
    for c0 in range(0, len(items), face_batch):
        ch = items[c0:c0 + face_batch]
        img, s01 = sample_chunk(m, [src[i] for i, _ in ch], [faces[i][k] for i, k in ch], [ref[i] for i, _ in ch], [ref_boxes[i] for i, _ in ch],
                                d['batch']['txt_emb'][[i for i, _ in ch]], d['x_T'][c0:c0 + len(ch)])
        imgs.append(img)
        srcs.append(s01)
    out = [p.clone() for p in src]
    img, s01 = torch.cat(imgs), torch.cat(srcs)
    for rank in range(max(len(f) for f in faces)):
        sel = [j for j, (_, k) in enumerate(items) if k == rank]
        photo.paste_photos([out[items[j][0]] for j in sel], [faces[items[j][0]][rank] for j in sel], img[sel], s01[sel], feather)
    return out


def overlap(a, b):
    return a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]


def test_group_photo_is_the_chain_of_the_calls(m, data):
    faces = faces_of(SRC_MAPS, data['src'], 4)
    assert [len(f) for f in faces] == [3, 1]
    f0 = faces[0]
    assert f0[0][2] >= f0[1][2] and overlap(f0[0], f0[2]) and not overlap(f0[0], f0[1]) and not overlap(f0[1], f0[2])      # largest first
    ref_boxes = [f[0] for f in faces_of(REF_MAPS, data['ref'], 1)]
    assert ref_boxes[0] == photo.grow_square_box((20 * 70 // PS, -(-51 * 70 // PS) - 1, 20, 50), 70, 64, 1.0)                # the LARGEST face
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    got, told = m.transfer_photos(data['src'], data['ref'], feather=3, x_T=data['x_T'], size=S, batch=data['batch'], max_faces=4, face_batch=3,
                                  return_faces=True)
    assert told == faces and m.face_parser.n == 2                                      # one parse per side, nothing per face
    m.reset_conditioning_cache()
    want = by_hand(m, data, faces, ref_boxes, 3, 3)
    for i, (g, w, p) in enumerate(zip(got, want, data['src'])):
        assert g.dtype == torch.uint8 and g.device.type == 'cuda' and tuple(g.shape) == tuple(p.shape)
        g, w, p = g.cpu().numpy(), w.cpu().numpy(), p.numpy()
        assert np.array_equal(g, w), f'photo {i}: {int((g != w).sum())} bytes differ from the chain of the calls'
        union = np.zeros(p.shape[:2], bool)
        for x0, y0, bw, bh in faces[i]:
            union[y0:y0 + bh, x0:x0 + bw] = True
            assert (g[y0:y0 + bh, x0:x0 + bw] != p[y0:y0 + bh, x0:x0 + bw]).mean() > 0.3           # every face was made up
        assert (~union).any() and np.array_equal(g[~union], p[~union])                  # every byte outside the faces' boxes is the photo's


def test_explicit_nested_boxes_need_no_parser(m, data):
    faces = faces_of(SRC_MAPS, data['src'], 4)
    ref_boxes = [f[0] for f in faces_of(REF_MAPS, data['ref'], 1)]
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    want = m.transfer_photos(data['src'], data['ref'], feather=2, x_T=data['x_T'], size=S, batch=data['batch'], max_faces=3, face_batch=8)
    m.face_parser = None
    m.reset_conditioning_cache()
    got = m.transfer_photos(data['src'], data['ref'], faces, ref_boxes, feather=2, x_T=data['x_T'], size=S, batch=data['batch'], max_faces=3)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_a_faceless_photo_comes_back_unchanged(m, data):
    m.face_parser = StubParser(torch.stack([EMPTY, SRC_MAPS[1]]), REF_MAPS)
    got, faces = m.transfer_photos(data['src'], data['ref'], x_T=data['x_T'][:1], size=S, batch=data['batch'], max_faces=4, return_faces=True)
    assert [len(f) for f in faces] == [0, 1]
    assert torch.equal(got[0].cpu(), data['src'][0]) and not torch.equal(got[1].cpu(), data['src'][1])
    m.face_parser = StubParser(torch.stack([EMPTY, EMPTY]), REF_MAPS)               # N = 0: nothing is sampled
    got, faces = m.transfer_photos(data['src'], data['ref'], size=S, batch=data['batch'], max_faces=4, return_faces=True)
    assert faces == [[], []] and all(torch.equal(g.cpu(), p) for g, p in zip(got, data['src']))
    m.face_parser = StubParser(SRC_MAPS, torch.stack([REF_MAPS[0], EMPTY]))
    with pytest.raises(ValueError, match='reference photo 1'):
        m.transfer_photos(data['src'], data['ref'], size=S, batch=data['batch'], max_faces=4)


def test_one_blob_photo_gives_the_single_box_calls_bytes(m, data):
    """on a photo with ONE component find_faces' box is find_boxes' box, and max_faces = 1 runs the same pass as the existing call"""
    src, ref, text, x_T = data['src'][1:], data['ref'][1:], {'txt_emb': data['batch']['txt_emb'][1:]}, data['x_T'][:1]
    m.face_parser = StubParser(SRC_MAPS[1:], REF_MAPS[1:])
    old = m.transfer_photos(src, ref, feather=3, x_T=x_T, size=S, batch=text)                                   # max_faces=None: find_boxes
    m.reset_conditioning_cache()
    m.face_parser = StubParser(SRC_MAPS[1:], REF_MAPS[1:])
    new = m.transfer_photos(src, ref, feather=3, x_T=x_T, size=S, batch=text, max_faces=1)
    assert torch.equal(old[0], new[0]) and not torch.equal(new[0].cpu(), src[0])


def test_max_faces_1_makes_up_the_largest_face_only(m, data):
    src, ref, text, x_T = data['src'][:1], data['ref'][:1], {'txt_emb': data['batch']['txt_emb'][:1]}, data['x_T'][:1]
    m.face_parser = StubParser(SRC_MAPS[:1], REF_MAPS[:1])
    got, faces = m.transfer_photos(src, ref, x_T=x_T, size=S, batch=text, max_faces=1, return_faces=True)
    (x0, y0, bw, bh), = faces[0]
    spanning, = fp.find_boxes(StubParser(SRC_MAPS[:1]), [src[0].to(DEV)], parse_size=PS)          # the existing path: ONE box around all three
    assert spanning != faces[0][0] and spanning[2] > bw
    g, p = got[0].cpu().numpy(), src[0].numpy()
    inside = np.zeros(p.shape[:2], bool)
    inside[y0:y0 + bh, x0:x0 + bw] = True
    assert np.array_equal(g[~inside], p[~inside]) and (g[inside] != p[inside]).mean() > 0.3
