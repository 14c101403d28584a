"""-m gpu: TestDiffuseModel.transfer_photos(guided_paste=...) on the small model and the stub parser of tests/test_gpu_model_faces.py.
The call is crop -> the same sampling pass -> the guided paste: every paste the call makes is watched (the photos before and after it,
the decoded samples and the source crops it was handed), and each must be, byte for byte, the numpy restatement
(tests/photo_guided_ref.py) of the guided paste on those inputs -- a plain box, max_faces = 2 with own_pixels, and align with rolled
faces.  Without guided_paste the bytes are those of the call without the keyword."""
import numpy as np
import pytest
import torch

import photo_guided_ref as gr
import photo_ref as pr
from makeupdiffuse_amd import photo
from test_gpu_model_faces import REF_MAPS, S, SRC_MAPS, StubParser, data, m, model  # noqa: F401  (fixtures: an instance for this module)

pytestmark = pytest.mark.gpu

FEATHER = 3
GUIDED = photo.GuidedPaste(1, 8.0)
SRC_BOXES, REF_BOXES = [(10, 20, 70, 70), (2, 0, 60, 60)], [(5, 3, 50, 50), (20, 10, 60, 60)]


@pytest.fixture()
def watched(monkeypatch):
    """every photo.paste_regions call of the test, as dicts of host copies; the call itself goes through"""
    calls = []
    real = photo.paste_regions

    def paste_regions(photos, regions, samples, src01, feather=8, weights=None, guided=None):
        rec = dict(before=[p.cpu().numpy().copy() for p in photos], regions=list(regions), t=samples.cpu().numpy().copy(),
                   s01=src01.cpu().numpy().copy(), feather=feather, w=None if weights is None else weights.cpu().numpy().copy(), guided=guided)
        out = real(photos, regions, samples, src01, feather, weights, guided)
        rec['after'] = [p.cpu().numpy().copy() for p in photos]
        calls.append(rec)
        return out
    monkeypatch.setattr(photo, 'paste_regions', paste_regions)
    return calls


def check_pastes(calls, guided):
    """every watched paste is the restatement's, on the bytes it found; -> the number of frame pastes among them"""
    frames = 0
    for c in calls:
        assert c['guided'] == guided and isinstance(c['guided'], photo.GuidedPaste)
        for j, r in enumerate(c['regions']):
            w = None if c['w'] is None else c['w'][j]
            box = tuple(r) if len(r) == 4 else photo.box_from_frame(r)
            if box is not None:
                want = gr.paste(c['before'][j], box, c['t'][j], c['s01'][j], c['feather'], guided.radius, guided.sigma, w)
            else:
                frames += 1
                want = gr.paste_frame(c['before'][j], tuple(r), c['t'][j], c['s01'][j], c['feather'], guided.radius, guided.sigma, w)[0]
            got = c['after'][j]
            assert np.array_equal(got, want), f'region {r}: {int((got != want).sum())} bytes differ from the restatement of the guided paste'
            assert not np.array_equal(got, c['before'][j])
    return frames


def test_a_plain_box_is_crop_sampling_and_the_guided_paste(m, data, watched):
    m.face_parser = None
    kw = dict(feather=FEATHER, x_T=data['x_T'][:2], size=S, batch=data['batch'])
    got = m.transfer_photos(data['src'], data['ref'], SRC_BOXES, REF_BOXES, guided_paste=GUIDED, **kw)
    assert len(watched) == 1 and check_pastes(watched, GUIDED) == 0
    c = watched[0]
    for i, (g, p, box) in enumerate(zip(got, data['src'], SRC_BOXES)):
        assert g.dtype == torch.uint8 and g.device.type == 'cuda'
        assert np.array_equal(c['before'][i], p.numpy()) and np.array_equal(g.cpu().numpy(), c['after'][i])
        # the crop the paste was handed is the restatement's crop of the photo: its guide is the bytes the model saw
        assert np.array_equal(c['s01'][i].view(np.uint32), pr.img01(pr.crop_resize_u8(p.numpy(), box, S)).view(np.uint32))
    # the same pass without the keyword, and with None: the bilinear paste of the same samples, byte for byte the same twice
    guided_calls = list(watched)
    del watched[:]
    m.reset_conditioning_cache()
    plain = m.transfer_photos(data['src'], data['ref'], SRC_BOXES, REF_BOXES, **kw)
    m.reset_conditioning_cache()
    none = m.transfer_photos(data['src'], data['ref'], SRC_BOXES, REF_BOXES, guided_paste=None, **kw)
    assert len(watched) == 2 and all(w['guided'] is None for w in watched)
    assert np.array_equal(watched[0]['t'].view(np.uint32), guided_calls[0]['t'].view(np.uint32))          # the same sampling pass
    for i, (a, b, p, box) in enumerate(zip(plain, none, data['src'], SRC_BOXES)):
        assert torch.equal(a, b) and not torch.equal(a, got[i])
        assert np.array_equal(a.cpu().numpy(), pr.paste(p.numpy(), box, watched[0]['t'][i], watched[0]['s01'][i], FEATHER))
    with pytest.raises(ValueError, match='GuidedPaste'):
        m.transfer_photos(data['src'], data['ref'], SRC_BOXES, REF_BOXES, guided_paste=(1, 8.0), **kw)


def test_group_photos_with_own_pixels_paste_every_rank_guided(m, data, watched):
    m.face_parser = StubParser(SRC_MAPS, REF_MAPS)
    got, faces = m.transfer_photos(data['src'], data['ref'], feather=FEATHER, x_T=data['x_T'][:3], size=S, batch=data['batch'], max_faces=2,
                                   own_pixels=True, own_feather=2, return_faces=True, guided_paste=GUIDED)
    assert [len(f) for f in faces] == [2, 1] and len(watched) == 2                     # one paste call per rank
    assert all(c['w'] is not None for c in watched) and check_pastes(watched, GUIDED) == 0
    assert np.array_equal(watched[0]['before'][0], data['src'][0].numpy())
    assert np.array_equal(watched[1]['before'][0], watched[0]['after'][0])               # rank 1 is pasted onto rank 0's result
    assert np.array_equal(got[0].cpu().numpy(), watched[1]['after'][0]) and np.array_equal(got[1].cpu().numpy(), watched[0]['after'][1])


def test_rolled_faces_are_pasted_guided_along_their_frames(m, data, watched):
    m.face_parser = None
    src_boxes = [[(20, 30, 50, 50, 30.0), (40, 60, 40, 40, -45.0)], [(8, 8, 48, 48)]]            # two rolled squares that stick out, and an upright box
    ref_boxes = [(10, 12, 40, 40, -20.0), (20, 10, 60, 60)]
    got, told = m.transfer_photos(data['src'], data['ref'], src_boxes, ref_boxes, feather=FEATHER, x_T=data['x_T'][:3], size=S, batch=data['batch'],
                                  max_faces=2, align=True, return_faces=True, guided_paste=GUIDED)
    assert len(watched) == 2 and check_pastes(watched, GUIDED) == 2                    # rank 0: a frame and a box in one call; rank 1: a frame
    assert len(watched[0]['regions']) == 2 and len(watched[1]['regions']) == 1
    assert np.array_equal(got[0].cpu().numpy(), watched[1]['after'][0]) and np.array_equal(got[1].cpu().numpy(), watched[0]['after'][1])
