"""-m gpu: teacher_warp in TestDiffuseModel on the small model of test_gpu_model_teacher.py (64 x 64 images, 8 x 8 latents, 5 steps): the
ground_truth row is teacher.pseudo_ground_truth's warped image, a teacher-started pass still equals the composition of the existing calls
bit for bit, and with the keyword off nothing moves."""
import numpy as np
import pytest
import torch

from gpu_util import DEV
from makeupdiffuse_amd import noise, teacher
from test_gpu_model_teacher import K, STEPS, TAU, DeviceCalls, Evaluations, build, by_hand, make_batch, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def plain():
    return build(teacher='hist')


@pytest.fixture(scope='module')
def model():
    return build(teacher='hist', teacher_warp=True)


def warp_batch(m, order=(0, 1)):
    b = make_batch(m, order)
    rng = np.random.RandomState(17)
    flat = np.stack([rng.choice(64 * 64, 20, replace=False) for _ in range(2)])
    lms = np.stack([flat // 64, flat % 64], 2).astype(np.float32)
    b[m.lms_key] = torch.from_numpy(lms[list(order)])
    b[m.ref_lms_key] = torch.from_numpy((lms + rng.uniform(-4, 4, lms.shape).astype(np.float32))[list(order)])
    return b


@pytest.mark.parametrize('warp', [True, {'eye': 1.0, 'lip': [0.0, 0.5]}])
def test_ground_truth_is_the_warped_teacher_image(model, plain, warp):
    m = model
    m.teacher_warp = warp
    try:
        m.reset_conditioning_cache()
        batch = warp_batch(m)
        log = m.log_results(batch, 0, seeds=5)
    finally:
        m.teacher_warp = True
    dev = lambda k: batch[k].to(DEV)
    x_p = teacher.pseudo_ground_truth(dev('src_img'), dev('ref_img'), dev(m.seg_key), dev(m.ref_seg_key), feather=2, lms_src=batch[m.lms_key],
                                      lms_ref=batch[m.ref_lms_key], warp=warp)[0]
    assert same(log['ground_truth'], x_p * 2.0 - 1.0)
    plain.reset_conditioning_cache()
    old = plain.log_results(make_batch(plain), 0, seeds=5)
    assert set(log) == set(old) and not same(log['ground_truth'], old['ground_truth'])
    # the rows built on x_p follow it: the reconstruction is the decoded encoding of THIS ground truth
    assert same(log['reconstruction'], m.decode_first_stage(m.get_z(log['ground_truth'], seeds=noise.as_seeds(5, 2))))
    assert not same(log['reconstruction'], old['reconstruction'])


@pytest.mark.parametrize('scale', [1.0, 9.0])
def test_a_teacher_started_pass_is_still_the_composition(model, scale):
    m = model
    m.unconditional_guidance_scale, m.teacher_start = scale, TAU
    try:
        assert teacher.start_steps(TAU, STEPS) == K
        sd = noise.as_seeds(21, 2)
        m.reset_conditioning_cache()
        with Evaluations(m) as ev:
            log = m.log_results(warp_batch(m), 0, seeds=sd)
        assert ev.calls == [('ddim', K)] * (1 if scale == 1.0 else 2), ev.calls
        m.reset_conditioning_cache()
        want = by_hand(m, warp_batch(m), log['ground_truth'], sd, scale)
        name = 'samples_latent' if scale == 1.0 else f'samples_cfg_scale_{scale:.2f}_latent'
        assert same(log[name], want) and same(log[name[:-7]], m.decode_first_stage(want))
    finally:
        m.unconditional_guidance_scale, m.teacher_start = 9, None


@pytest.mark.parametrize('start', [None, TAU])
def test_with_the_keyword_off_nothing_moves(model, plain, start):
    model.teacher_warp = None
    model.teacher_start = plain.teacher_start = start
    try:
        out, calls = [], []
        for m, batch in ((plain, make_batch(plain)), (model, warp_batch(model))):          # (landmarks in the batch change nothing either)
            m.reset_conditioning_cache()
            with Evaluations(m) as ev, DeviceCalls(m) as dc:
                out.append(m.log_results(batch, 0, seeds=5))
            calls.append((list(ev.calls), list(dc.calls)))
    finally:
        model.teacher_warp = True
        model.teacher_start = plain.teacher_start = None
    a, b = out
    assert sorted(a) == sorted(b) and 'ground_truth' in a
    for k in a:
        assert same(a[k], b[k]), k
    assert calls[0] == calls[1]


def test_missing_landmarks_are_refused_before_any_launch(model):
    m = model
    b = warp_batch(m)
    del b[m.ref_lms_key]
    with DeviceCalls(m) as dc, pytest.raises(ValueError, match='landmarks'):
        m.log_results(b, 0, seeds=1)
    assert not dc.calls, dc.calls
