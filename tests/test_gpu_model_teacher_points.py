"""-m gpu: teacher_points='masks' in TestDiffuseModel on the small model of test_gpu_model_teacher.py (64 x 64 images, 8 x 8 latents, 5
steps): the ground_truth row is the warped teacher image with control points from the masks and needs no landmark keys;
transfer_photos(teacher_start=) takes teacher_warp with it and runs exactly k evaluations; without it the refusal stands."""
import pytest
import torch

from gpu_util import DEV
from makeupdiffuse_amd import teacher
from test_gpu_model_teacher import K, TAU, Evaluations, build, make_batch, photos, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model():
    return build(teacher='hist', teacher_warp=True, teacher_points='masks')


@pytest.mark.parametrize('dirs', [16, 8])
def test_ground_truth_needs_no_landmark_keys(model, dirs):
    m = model
    m.teacher_point_dirs = dirs
    try:
        m.reset_conditioning_cache()
        batch = make_batch(m)
        assert m.lms_key not in batch and m.ref_lms_key not in batch
        log = m.log_results(batch, 0, seeds=5)
    finally:
        m.teacher_point_dirs = 16
    dev = lambda k: batch[k].to(DEV)
    args = (dev('src_img'), dev('ref_img'), dev(m.seg_key), dev(m.ref_seg_key))
    x_p = teacher.pseudo_ground_truth(*args, feather=2, warp=True, points='masks', point_dirs=dirs)[0]
    assert same(log['ground_truth'], x_p * 2.0 - 1.0)
    assert not same(x_p, teacher.pseudo_ground_truth(*args, feather=2)[0])          # the warped term is in it


def test_transfer_photos_takes_the_warped_teacher_with_mask_points(model):
    d = photos()
    m = model
    kw = dict(src_segs=d['ssegs'], ref_segs=d['rsegs'], feather=3, size=64, batch=d['batch'], seeds=40, teacher_start=TAU)
    m.reset_conditioning_cache()
    with Evaluations(m) as ev:
        got = m.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], **kw)
    assert ev.calls == [('ddim', K)]
    assert len(got) == 2 and all(g.dtype == torch.uint8 and tuple(g.shape) == tuple(p.shape) for g, p in zip(got, d['src']))
    m.reset_conditioning_cache()
    again = m.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # the warped term reaches the photos: the same call with the alpha = 0 teacher gives other bytes
    m.teacher_warp = None
    try:
        m.reset_conditioning_cache()
        plain = m.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], **kw)
    finally:
        m.teacher_warp = True
    assert not any(torch.equal(a, b) for a, b in zip(got, plain))
    # without 'masks' the refusal and its text stand
    m.teacher_points = None
    try:
        with pytest.raises(ValueError, match='teacher_start is not combined with teacher_warp \\(crops carry no landmarks'):
            m.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], **kw)
    finally:
        m.teacher_points = 'masks'
