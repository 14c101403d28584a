"""-m gpu: TestDiffuseModel.transfer_photos(max_faces=..., align=True) on the small model and the stub parser of
tests/test_gpu_model_faces.py (the parser's label maps are fixed, so the faces and their rolls are known; everything behind the maps
-- components, face frames, owner map, crops, sampling, pastes -- runs on the device).  Upright faces: the bytes of align=False.
Caller boxes with an angle: only the rotated squares change.  Rolled faces from the parser with own_pixels: the call runs and a pixel
no pasted face owns keeps its byte."""
import numpy as np
import pytest
import torch

import owner_ref as orf
import photo_frame_ref as fr
from gpu_util import DEV
from makeupdiffuse_amd import face_parser as fp
from makeupdiffuse_amd import photo
from test_gpu_model_faces import PS, REF_MAPS, S, SRC_MAPS, StubParser, data, m, model  # noqa: F401  (fixtures: an instance for this module)

pytestmark = pytest.mark.gpu

FEATHER = 3


def rolled_map():
    """three faces on the PS x PS map, largest first: rolled +25 and -20 degrees, and a small upright one between them"""
    lab = np.zeros((PS, PS), np.uint8)
    fr.draw_face(lab, 18, 20, 8, 10, 25.0)
    fr.draw_face(lab, 47, 18, 6, 8, -20.0)
    fr.draw_face(lab, 33, 32, 4, 5, 0.0)
    return torch.from_numpy(lab)


def test_upright_faces_give_the_bytes_of_the_unaligned_call(m, data):
    """the stub's blobs have no eyes: every frame is its box, and the aligned call is the present path call for call"""
    kw = dict(feather=FEATHER, x_T=data['x_T'], size=S, batch=data['batch'], max_faces=4, face_batch=3, return_faces=True)
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    plain, boxes = m.transfer_photos(data['src'], data['ref'], **kw)
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    m.reset_conditioning_cache()
    got, frames = m.transfer_photos(data['src'], data['ref'], align=True, **kw)
    assert [[photo.box_from_frame(f) for f in fl] for fl in frames] == boxes and all(f.s == 0.0 for fl in frames for f in fl)
    assert all(torch.equal(g, p) for g, p in zip(got, plain)) and not torch.equal(got[0].cpu(), data['src'][0])
    # the same with caller boxes that carry an angle of 0, and with plain 4-tuples
    ref_boxes = [f[0] for f in fp.find_faces(StubParser(REF_MAPS), [p.to(DEV) for p in data['ref']], max_faces=1, parse_size=PS)]
    for tilt in ((0.0,), ()):
        m.face_parser = None
        m.reset_conditioning_cache()
        again = m.transfer_photos(data['src'], data['ref'], [[b + tilt for b in bl] for bl in boxes], [b + tilt for b in ref_boxes], align=True,
                                  **dict(kw, return_faces=False))
        assert all(torch.equal(g, p) for g, p in zip(again, plain))
    with pytest.raises(ValueError, match='align only applies with max_faces'):
        m.transfer_photos(data['src'], data['ref'], [b[0] for b in boxes], ref_boxes, align=True, size=S)
    with pytest.raises(ValueError, match='max_faces'):                            # a 5-tuple is a box only with align
        m.transfer_photos(data['src'], data['ref'], [[(10, 10, 40, 40, 15.0)], []], ref_boxes, size=S, max_faces=2)
    with pytest.raises(ValueError, match='not square'):
        m.transfer_photos(data['src'], data['ref'], [[(10, 10, 40, 30, 15.0)], []], ref_boxes, size=S, max_faces=2, align=True)


def test_caller_boxes_with_angles_change_only_their_rotated_squares(m, data):
    m.face_parser = None
    src_boxes = [[(20, 30, 50, 50, 30.0), (40, 60, 40, 40, -45.0)], [(8, 8, 48, 48, 17.0)]]          # 120 x 90 and 64 x 64: squares that stick out
    ref_boxes = [(10, 12, 40, 40, -20.0), (20, 10, 60, 60)]
    got, told = m.transfer_photos(data['src'], data['ref'], src_boxes, ref_boxes, feather=FEATHER, x_T=data['x_T'][:3], size=S, batch=data['batch'],
                                  max_faces=2, align=True, return_faces=True)
    assert told == [[photo.frame_from_box(b[:4], b[4]) for b in bl] for bl in src_boxes]
    for g, p, fl in zip(got, data['src'], told):
        g, p = g.cpu().numpy(), p.numpy()
        H, W = p.shape[:2]
        inside = np.zeros((H, W), bool)
        for f in fl:
            inside |= fr.inside_mask(H, W, f)
        assert 0 < inside.sum() < H * W
        assert np.array_equal(g[~inside], p[~inside]), 'bytes outside every rotated square must be the photo\'s own'
        assert (g[inside] != p[inside]).mean() > 0.3
    # the rotated crop is what the model saw: another angle, other bytes
    m.reset_conditioning_cache()
    other = m.transfer_photos(data['src'], data['ref'], [[b[:4] + (b[4] + 10.0,) for b in bl] for bl in src_boxes], ref_boxes, feather=FEATHER,
                              x_T=data['x_T'][:3], size=S, batch=data['batch'], max_faces=2, align=True)
    assert not torch.equal(other[0], got[0])


def test_rolled_faces_from_the_parser_with_own_pixels(m, data):
    g = torch.Generator().manual_seed(733)
    src = [torch.randint(0, 256, (128, 128, 3), generator=g, dtype=torch.uint8)]
    ref = [data['ref'][0]]
    maps = rolled_map()[None]
    text = {'txt_emb': data['batch']['txt_emb'][:1]}
    dev_src = [p.to(DEV) for p in src]
    frames, owner = fp.find_faces(StubParser(maps), dev_src, max_faces=2, parse_size=PS, return_owner=True, oriented=True)
    assert len(frames[0]) == 2 and all(isinstance(f, photo.Frame) and f.s != 0.0 for f in frames[0])
    for f, want in zip(frames[0], (25.0, -20.0)):
        assert abs(np.degrees(np.arctan2(f.s, f.c)) - want) <= 4.0                # tiny eyes on a 64 x 64 map: a coarse check of the sign
    m.face_parser = StubParser(maps, REF_MAPS[:1])
    got, told = m.transfer_photos(src, ref, feather=FEATHER, x_T=data['x_T'][:2], size=S, batch=text, max_faces=2, own_pixels=True, own_feather=2,
                                  align=True, return_faces=True)
    assert told[0] == frames[0] and m.face_parser.n == 2
    out, p = got[0].cpu().numpy(), src[0].numpy()
    o = owner[0].cpu().numpy()
    w = [orf.weight_at_photo(orf.weights(o, k, 2), 128, 128) for k in range(2)]
    inside = [fr.inside_mask(128, 128, f) for f in frames[0]]
    # inside rank 0's square, where rank 0 owns nothing and rank 1 either owns nothing or does not reach: the third face's pixels
    kept = inside[0] & (w[0] == 0) & ((w[1] == 0) | ~inside[1])
    assert kept.sum() > 100 and np.array_equal(out[kept], p[kept])
    own0 = inside[0] & (w[0] == 1)
    assert (out[own0] != p[own0]).mean() > 0.3                                   # while rank 0's own pixels were made up
    assert np.array_equal(out[~(inside[0] | inside[1])], p[~(inside[0] | inside[1])])
    # without own_pixels the kept pixels are repainted from rank 0's crop
    m.face_parser = StubParser(maps, REF_MAPS[:1])
    m.reset_conditioning_cache()
    loose = m.transfer_photos(src, ref, feather=FEATHER, x_T=data['x_T'][:2], size=S, batch=text, max_faces=2, align=True)[0].cpu().numpy()
    assert (loose[kept] != p[kept]).any()
