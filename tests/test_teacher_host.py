"""CPU: the histogram-matching teacher's definition (tests/teacher_ref.py, the restatement mkd_pgt_compose is held to on the device) and
the host-side rules around it: the step count of a teacher-started pass, the seeded timestep of the sample_ddmp row, the strengths and
keyword checks, and the refusals of the model and of the C entry that need no device."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import teacher_ref as tr
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd import noise, teacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'hist_match_ref.npz'))
IDENT = np.tile(np.arange(256, dtype=np.uint8), (4, 1, 3, 1))          # [4, 1, 3, 256]


# ---- 1. region ids and window counts ---------------------------------------------------------------------------------------------
def test_priority_on_overlapping_masks():
    m = np.zeros((4, 1, 1, 16), dtype=np.uint8)          # planes lip, skin, eye_left, eye_right: every subset of the four, one per pixel
    for p in range(16):
        for plane in range(4):
            m[plane, 0, 0, p] = (p >> plane) & 1
    ids = tr.region_ids(m)[0, 0]
    for p in range(16):
        lip, skin, el, er = p & 1, (p >> 1) & 1, (p >> 2) & 1, (p >> 3) & 1
        assert ids[p] == (1 if lip else 2 if el else 3 if er else 4 if skin else 0), p
    m[:, 0, 0, :] *= 200          # any non-zero value is inside
    assert np.array_equal(tr.region_ids(m)[0, 0], ids)


@pytest.mark.parametrize('F', [0, 1, 3, 8])
def test_counts_sum_to_at_most_K_and_the_corner_window(F):
    rng = np.random.RandomState(F)
    m = (rng.rand(4, 2, 11, 13) < 0.4).astype(np.uint8)
    ids = tr.region_ids(m)
    c = tr.window_counts(ids, F)
    K = (2 * F + 1) ** 2
    assert c.sum(0).max() <= K and c.min() >= 0
    # brute force at every pixel: only pixels inside the image count
    for y, x in ((0, 0), (0, 12), (10, 0), (10, 12), (5, 6)):
        win = ids[:, max(y - F, 0):y + F + 1, max(x - F, 0):x + F + 1]
        for r in range(4):
            assert np.array_equal(c[r][:, y, x], (win == r + 1).sum((1, 2)))
    # all four masks full: every pixel is lip; the corner sees (F + 1)^2 of K
    full = tr.window_counts(tr.region_ids(np.ones((4, 1, 20, 20), dtype=np.uint8)), F)
    assert full[0][0, 0, 0] == (F + 1) ** 2 and full[0][0, 10, 10] == K and not full[1:].any()


# ---- 2. the composition ----------------------------------------------------------------------------------------------------------
def test_hard_composition_equals_the_reference_pinned_matched_values():
    """F = 0, a = 1 on golden case 0: inside region r the output is (matched_r + (v - i)) / 255 with the REFERENCE's matched values
    (the golden file's, term 2 r = source matched to reference), elsewhere the clamped source"""
    A = GOLD['c0_img_a'].astype(np.float32) / np.float32(65535.0)
    masks = GOLD['c0_mask_a'][:, None]                                     # [4, 1, H, W]
    tables = GOLD['c0_tables'][0::2][:, None]                              # terms 0, 2, 4, 6: A matched to B per region
    out = tr.compose(A[None], masks, tables, None, 0)[0]
    ids = tr.region_ids(masks)[0]
    v = tr.values(A)
    frac = v.astype(np.float64) - v.astype(np.int64)
    want = v.astype(np.float64)
    for r in range(4):
        inside = ids == r + 1
        assert inside.any()
        matched = GOLD['c0_matched'][2 * tr.ID_PLANE[r]].astype(np.float64)
        assert not matched[:, GOLD['c0_mask_a'][tr.ID_PLANE[r]] == 0].any()
        want = np.where(inside[None], matched + frac, want)
    assert np.array_equal(out, np.clip(want / 255.0, 0, 1).astype(np.float32))
    assert np.array_equal(out[:, ids == 0], (v.astype(np.float64) / 255.0).astype(np.float32)[:, ids == 0])


def test_identity_tables_and_zero_strength_give_the_source():
    rng = np.random.RandomState(1)
    k = rng.randint(0, 256, (2, 3, 9, 14))
    src = (k / 255).astype(np.float32)                                     # exact k / 255 values
    assert np.array_equal(tr.values(src), k.astype(np.float32))            # (every k / 255 lands on its own bin)
    masks = (rng.rand(4, 2, 9, 14) < 0.5).astype(np.uint8)
    tables = rng.randint(0, 256, (4, 2, 3, 256)).astype(np.uint8)
    for F in (0, 2, 8):
        assert np.array_equal(tr.compose(src, masks, np.repeat(IDENT, 2, 1), None, F), src)            # bit for bit
        assert np.array_equal(tr.compose(src, masks, tables, np.zeros((2, 4), np.float32), F), src)
        assert not np.array_equal(tr.compose(src, masks, tables, None, F), src)
    # any other value: the clamped source within one fp32 ulp (v / 255 after v = s 255, each rounded once)
    wild = rng.uniform(-0.2, 1.2, src.shape).astype(np.float32)
    got = tr.compose(wild, masks, tables, np.zeros((2, 4), np.float32), 3)
    assert np.abs(got - np.clip(wild, 0, 1)).max() <= 2.0 ** -23
    assert tr.compose(np.full((1, 3, 2, 2), np.nan, np.float32), masks[:, :1, :2, :2], tables[:, :1], None, 0).max() <= 1.0          # NaN -> bin 0
    zero = tr.compose(np.full((1, 3, 2, 2), -0.0, np.float32), masks[:, :1, :2, :2], np.repeat(IDENT, 1, 1), None, 0)
    assert not zero.any() and not np.signbit(zero).any()                                                                              # -0 -> +0


def test_constant_region_maps_to_the_reference_constant_exactly():
    H = W = 12
    seg_s, seg_r = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    seg_s[2:6, 3:9] = 7
    seg_r[5:9, 1:7] = 9
    cs, cr = np.array([40, 120, 200]), np.array([250, 3, 77])
    src = np.full((3, H, W), 0.5, np.float32)
    ref = np.full((3, H, W), 0.25, np.float32)
    src[:, seg_s == 7] = (cs / 255).astype(np.float32)[:, None]
    ref[:, seg_r == 9] = (cr / 255).astype(np.float32)[:, None]
    out, tables, counts, masks = tr.pseudo_ground_truth(src[None], ref[None], seg_s[None], seg_r[None], None, 0)
    assert counts[0, 0].tolist() == [24, 24] and not counts[1:].any()
    for c in range(3):
        assert np.all(out[0, c][seg_s == 7] == np.float32(cr[c] / 255))
    assert np.array_equal(out[0][:, seg_s != 7], src[:, seg_s != 7])          # the empty regions have identity tables


def test_strength_and_feather_scale_the_change():
    src, ref, ss, rs = tr.synthetic_pairs()
    full, tables, counts, masks = tr.pseudo_ground_truth(src, ref, ss, rs, None, 0)
    half = tr.compose(src, masks, tables, np.full((3, 4), 0.5, np.float32), 0)
    assert np.abs((half.astype(np.float64) - src) - (full.astype(np.float64) - src) / 2).max() <= 2.0 ** -22
    a = np.ones((3, 4), np.float32)
    a[:, 0] = 0                                                             # lips off: lip pixels are what a = 0 gives everywhere
    keep = tr.compose(src, masks, tables, np.zeros((3, 4), np.float32), 0)
    assert np.abs(keep - src).max() <= 2.0 ** -23
    lip_off = tr.compose(src, masks, tables, a, 0)
    ids = tr.region_ids(masks)
    assert np.array_equal(lip_off.transpose(1, 0, 2, 3)[:, ids == 1], keep.transpose(1, 0, 2, 3)[:, ids == 1])
    assert np.array_equal(lip_off.transpose(1, 0, 2, 3)[:, ids != 1], full.transpose(1, 0, 2, 3)[:, ids != 1])
    # the feathered image reaches past the regions and fades towards the border
    soft = tr.compose(src, masks, tables, None, 2)
    changed = np.abs(soft - keep).max(1) > 0
    assert (changed & (ids == 0)).any() and np.array_equal(changed & ~(tr.window_counts(ids, 2).sum(0) > 0), np.zeros_like(changed))


def test_teacher_lowers_the_score_on_the_synthetic_pairs():
    """the condition of the device test of the same name, on the restatement alone"""
    src, ref, ss, rs = tr.synthetic_pairs()
    base = tr.transfer_score(src, ref, ss, rs)
    for F in (0, 2):
        x_p, _, counts, _ = tr.pseudo_ground_truth(src, ref, ss, rs, None, F)
        assert counts.min() > 0
        assert (tr.transfer_score(x_p, ref, ss, rs) < base).all()


# ---- 3. host rules ---------------------------------------------------------------------------------------------------------------
def test_start_steps_rule():
    assert teacher.start_steps(1e-9, 50) == 1 and teacher.start_steps(0.001, 4) == 1          # tau -> 0: one evaluation
    assert teacher.start_steps(1.0, 50) == 50 and teacher.start_steps(1, 1) == 1
    assert teacher.start_steps(0.6, 50) == 30 and teacher.start_steps(0.6, 5) == 3
    assert teacher.start_steps(0.5, 5) == 2 and teacher.start_steps(0.5, 7) == 4 and teacher.start_steps(0.5, 3) == 2          # ties to even
    for S in (1, 4, 5, 50):
        for tau in (0.01, 0.3, 0.5, 0.77, 1.0):
            assert teacher.start_steps(tau, S) == tr.start_steps(tau, S) and 1 <= teacher.start_steps(tau, S) <= S
    for bad in (0, 0.0, -0.1, 1.0001, None, 'x', True, float('nan')):
        with pytest.raises(ValueError):
            teacher.start_steps(bad, 10)


def test_seeded_timestep_is_repeatable_and_position_independent():
    sd = noise.as_seeds([11, 2 ** 64 - 1, 0, 11], 4, subs=[0, 5, 0, 1])
    t = noise.teacher_timesteps(sd, 0, 1000)
    assert t == noise.teacher_timesteps(sd, 0, 1000) and all(0 <= v < 1000 for v in t)
    assert t[0] != t[3]                                                     # the sub-stream counts
    perm = [2, 0, 3, 1]
    assert noise.teacher_timesteps(sd.take(perm), 0, 1000) == [t[i] for i in perm]
    assert noise.teacher_timesteps(noise.as_seeds(11, 1), 0, 1000) == [t[0]]          # subs None = all 0
    lo = noise.teacher_timesteps(noise.as_seeds(0, 256), 400, 1000)
    assert min(lo) >= 400 and max(lo) < 1000 and len(set(lo)) > 100
    assert noise.teacher_timesteps(sd, 999, 1000) == [999] * 4
    # the written-down function, once by hand
    z = (11 + 0x9E3779B97F4A7C15) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert t[0] == (z ^ (z >> 31)) % 1000
    for t_min in (-1, 1000):
        with pytest.raises(ValueError):
            noise.teacher_timesteps(sd, t_min, 1000)
    assert noise.STREAM_TEACHER == 4 and noise.STREAM_TEACHER not in (noise.STREAM_START, noise.STREAM_ETA, noise.STREAM_BLEND, noise.STREAM_POSTERIOR)


def test_strength_rows_forms_and_refusals():
    assert teacher.strength_rows(None, 3) is None
    r = teacher.strength_rows({'lip': 0.5, 'eye': [0.0, 1.0]}, 2)
    assert r.dtype == torch.float32 and r.tolist() == [[0.5, 1.0, 0.0, 0.0], [0.5, 1.0, 1.0, 1.0]]          # lip, skin, eye_left, eye_right
    t = torch.tensor([[0.0, 0.25, 0.5, 1.0]])
    assert torch.equal(teacher.strength_rows(t, 1), t) and torch.equal(teacher.strength_rows(t.numpy(), 1), t)
    for bad in ({'lip': 1.5}, {'skin': -0.1}, {'eye': float('nan')}, {'nose': 1.0}, {'lip': [1.0, 1.0, 1.0]}, torch.ones(2, 3), torch.full((2, 4), 2.0)):
        with pytest.raises(ValueError):
            teacher.strength_rows(bad, 2)
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError):
            teacher.check_feather(bad)
    assert teacher.check_feather(0) == 0 and teacher.check_feather(8) == 8


def test_no_cpu_path():
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(mlib.MkdError):
        teacher.pseudo_ground_truth(x, x, torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_c_entry_refuses_bad_arguments_without_a_device():
    lib = mlib.load()
    buf = (C.c_float * 4096)()
    src, out = C.addressof(buf), C.addressof(buf) + 4 * 2048
    mbuf = (C.c_uint8 * 4096)()
    m = C.addressof(mbuf)
    call = lambda **kw: lib.mkd_pgt_compose(*[C.c_void_p(v) if k in ('src', 'masks', 'tables', 'strengths', 'out') else v for k, v in
                                              {**dict(src=src, masks=m, tables=m, strengths=None, n=1, H=8, W=8, feather=2, out=out), **kw}.items()], None)
    for kw in (dict(src=None), dict(masks=None), dict(tables=None), dict(out=None), dict(n=0), dict(n=65536), dict(H=0), dict(W=0), dict(H=4097, W=4096),
               dict(feather=-1), dict(feather=9), dict(out=src), dict(out=src + 4 * 100), dict(src=src + 2), dict(out=out + 1), dict(strengths=src + 1)):
        assert call(**kw) == -1 and lib.mkd_last_error(), kw          # MKD_ERR_ARG
    assert lib.mkd_pgt_launches() == 1


# ---- 4. the model's keyword checks and refusals, on a stand-in engine (the pattern of test_sample_extras_host.py) ---------------------
def _model(**attrs):
    from makeupdiffuse_amd.config import create_model
    m = create_model(os.path.join(ROOT, 'diffmodels', 'test_diffusion_makeup.yaml'))

    def no_engine():
        raise AssertionError('the engine was reached: the refusal came too late')
    m._require_engine = no_engine
    m.save_images = False
    m.ddim_steps = 10
    for k, v in {'teacher': 'hist', **attrs}.items():
        setattr(m, k, v)
    return m


def _batch(m, segs=True, B=2):
    g = torch.Generator().manual_seed(5)
    b = {'src_img': torch.rand(B, 3, 16, 16, generator=g), 'ref_img': torch.rand(B, 3, 16, 16, generator=g),
         'txt_emb': torch.randn(B, 77, m.net_config.context_dim, generator=g)}
    if segs:
        b[m.seg_key] = torch.ones(B, 16, 16, dtype=torch.uint8)
        b[m.ref_seg_key] = torch.ones(B, 16, 16, dtype=torch.uint8)
    return b


def test_constructor_keyword_checks():
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    for bad in (dict(teacher='elegant'), dict(teacher='hist', teacher_feather=9), dict(teacher='hist', teacher_feather=-1),
                dict(teacher_start=0.5), dict(teacher='hist', teacher_start=0.0), dict(teacher='hist', teacher_start=1.5),
                dict(teacher='hist', teacher_t_min=-1), dict(teacher='hist', teacher_t_min=0.5)):
        with pytest.raises(ValueError):
            TestDiffuseModel(**bad)                          # (checked before anything is built)


def test_teacher_needs_both_label_maps_and_says_so():
    m = _model()
    for drop in (m.seg_key, m.ref_seg_key):
        b = _batch(m)
        del b[drop]
        with pytest.raises(ValueError, match='label maps of the source and of the reference'):
            m.log_results(b, 0)
    m = _model(teacher_t_min=m.num_timesteps)
    with pytest.raises(ValueError, match='teacher_t_min'):
        m.log_results(_batch(m), 0)


@pytest.mark.parametrize('attrs,kw,names', [
    (dict(), dict(x_T=torch.zeros(2, 4, 2, 2)), 'x_T'),
    (dict(fix_background=True), {}, 'fix_background'),
    (dict(denoise_rows=True), {}, 'denoise_rows'),
    (dict(guidance_rescale=0.5), {}, 'guidance_rescale'),
    (dict(ddim_eta=0.3), {}, 'ddim_eta'),
])
def test_teacher_start_refusals_name_the_combination_before_the_engine(attrs, kw, names):
    m = _model(teacher_start=0.6, **attrs)
    with pytest.raises(ValueError, match=names):
        m.log_results(_batch(m), 0, **kw)


def test_teacher_start_is_refused_by_transfer_specs_video_and_photos():
    m = _model(teacher_start=0.6)
    with pytest.raises(ValueError, match='transfer_specs'):
        m.transfer_specs(_batch(m), [])
    frame = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='video'):
        m.video_session(frame)
    with pytest.raises(ValueError, match='video'):
        m.transfer_video([frame, frame], frame)
    with pytest.raises(ValueError, match='interpolate'):
        m.interpolate(_batch(m), [0.0, 1.0])
    with pytest.raises(ValueError, match='transfer_regions'):
        m.transfer_regions(_batch(m), {'lip': 'ref_img'})
    m = _model()
    with pytest.raises(ValueError, match='video'):
        m.video_session(frame, teacher_start=0.5)
    with pytest.raises(ValueError, match='video'):
        m.transfer_video([frame], frame, teacher_start=0.5)
    photo = [torch.zeros(32, 32, 3, dtype=torch.uint8)]
    box = [(0, 0, 32, 32)]
    seg = [torch.zeros(32, 32, dtype=torch.uint8)]
    with pytest.raises(ValueError, match='src_segs and ref_segs'):
        m.transfer_photos(photo, photo, box, box, src_segs=seg, teacher_start=0.5)
    with pytest.raises(ValueError, match='x_T'):
        m.transfer_photos(photo, photo, box, box, src_segs=seg, ref_segs=seg, teacher_start=0.5, x_T=torch.zeros(1, 4, 4, 4))
    for bad in (dict(teacher_start=1.5), dict(teacher_start=0.5, teacher_feather=9), dict(teacher_start=0.5, teacher_strengths={'lip': 2.0}),
                dict(ref_segs=seg), dict(teacher_feather=3), dict(teacher_strengths={'lip': 0.5})):
        with pytest.raises(ValueError):
            m.transfer_photos(photo, photo, box, box, src_segs=seg, **bad)
    m.fix_background = True
    with pytest.raises(ValueError, match='fix_background'):
        m.transfer_photos(photo, photo, box, box, src_segs=seg, ref_segs=seg, teacher_start=0.5)


def test_cli_refuses_teacher_start_where_the_pass_would_not_start_from_it():
    import subprocess
    cli = [sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--teacher', 'hist', '--teacher-start', '0.5']
    for more, word in ((['--fix-background'], '--fix-background'), (['--guidance-rescale', '0.5'], '--guidance-rescale')):
        r = subprocess.run(cli + more, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and f'--teacher-start is not combined with {word}' in r.stderr, (more, r.stderr[-400:])
    r = subprocess.run(cli[:2] + ['--teacher-start', '0.5'], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'only apply with --teacher hist' in r.stderr
