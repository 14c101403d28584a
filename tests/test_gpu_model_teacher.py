"""-m gpu: the histogram-matching teacher in TestDiffuseModel on a small model (64 x 64 images, 8 x 8 latents, 5 steps): with the keywords
off nothing moves; teacher='hist' adds exactly the reference's rows; teacher_start runs k = round(tau S) evaluations from the diffused
teacher latent and equals the composition of the existing calls bit for bit; transfer_photos(teacher_start=) on synthetic photos."""
import numpy as np
import pytest
import torch

import teacher_ref as tr
import vae_encoder_ref as enc_ref
from gpu_util import DEV, assert_close_bf16
from makeupdiffuse_amd import noise, teacher
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from oracle import nets, vae

pytestmark = pytest.mark.gpu

NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])      # f = 8
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))
STEPS, TAU, K = 5, 0.6, 3
NEW = {'ground_truth', 'reconstruction', 'sample_ddmp'}


def build(**kw):
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True,
                         ddim_steps=STEPS, unconditional_guidance_scale=9, **kw)
    m.load_state_dict({**nets.init_state_dict(OCFG, seed=31), **vae.init_state_dict(vcfg, seed=32), **enc_ref.init_state_dict(vcfg, seed=33)})
    m.cuda(0)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(34))
    m.save_images = False
    return m


@pytest.fixture(scope='module')
def base():
    return build()


@pytest.fixture(scope='module')
def model():
    return build(teacher='hist')


def make_batch(m, order=(0, 1)):
    src, ref, ss, rs = tr.synthetic_pairs(n=2, size=64)
    idx = list(order)
    g = torch.Generator().manual_seed(9)
    txt = torch.randn(2, 77, 64, generator=g)
    return {'src_img': torch.from_numpy(src[idx]), 'ref_img': torch.from_numpy(ref[idx]), 'txt_emb': txt[idx],
            m.seg_key: torch.from_numpy(ss[idx]), m.ref_seg_key: torch.from_numpy(rs[idx])}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


class Evaluations:
    """records (solver, table entries) of every in-library loop the model runs"""

    def __init__(self, m):
        self.m, self.calls = m, []

    def __enter__(self):
        inner = self.m._sample_loop

        def hook(solver, x_latent, cond, tables, *a, **k):
            self.calls.append((solver, len(tables[0])))
            return inner(solver, x_latent, cond, tables, *a, **k)
        self.m._sample_loop = hook
        return self

    def __exit__(self, *exc):
        del self.m._sample_loop


class DeviceCalls:
    """records the name of every call that can put work on the device: every public method of the model's MkdEngine and the libmkd
    wrappers of makeup_score / teacher / noise.  libmkd keeps no running launch counter; a call's launches are a function of its
    arguments, so two runs with the same call list and the same bytes out made the same launches"""

    def __init__(self, m):
        self.m, self.calls, self.undo = m, [], []

    def _wrap(self, owner, name, tag):
        inner = getattr(owner, name)

        def hook(*a, **k):
            self.calls.append(tag)
            return inner(*a, **k)
        had = name in vars(owner)
        setattr(owner, name, hook)
        self.undo.append((owner, name, inner if had else None))

    def __enter__(self):
        from makeupdiffuse_amd import makeup_score as ms
        eng = self.m.engine
        for name in dir(type(eng)):
            if not name.startswith('_') and callable(getattr(type(eng), name)) and not isinstance(getattr(type(eng), name), property):
                self._wrap(eng, name, 'engine.' + name)
        for mod, names in ((ms, ('region_mask', 'histogram_match')), (teacher, ('compose',)), (noise, ('_fill',))):
            for name in names:
                self._wrap(mod, name, f'{mod.__name__.rsplit(".", 1)[-1]}.{name}')
        return self

    def __exit__(self, *exc):
        for owner, name, inner in reversed(self.undo):
            if inner is None:
                delattr(owner, name)
            else:
                setattr(owner, name, inner)


@pytest.mark.parametrize('seeds', [None, 5])
def test_without_the_teacher_nothing_moves(base, model, seeds):
    model.teacher = None
    try:
        out, states = [], []
        for m in (base, model):
            m.reset_conditioning_cache()
            torch.manual_seed(3)
            with Evaluations(m) as ev, DeviceCalls(m) as dc:
                out.append(m.log_results(make_batch(m), 0, seeds=seeds))
            states.append((torch.get_rng_state(), torch.cuda.get_rng_state(0), list(ev.calls), list(dc.calls)))
    finally:
        model.teacher = 'hist'
    a, b = out
    assert sorted(a) == sorted(b) == ['control_ref', 'control_src', 'samples', 'samples_cfg_scale_9.00', 'samples_cfg_scale_9.00_latent',
                                      'samples_latent']
    for k in a:
        assert same(a[k], b[k]), k
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])          # the same draws from the torch generators
    assert states[0][2] == states[1][2] == [('ddim', STEPS), ('ddim', STEPS)]
    # the same device calls in the same order, and none of the teacher's
    assert states[0][3] == states[1][3] and states[0][3].count('engine.sample') == 2
    assert not [c for c in states[1][3] if c.startswith(('teacher.', 'makeup_score.')) or c == 'engine.encode']


@pytest.mark.parametrize('score', [False, True])
def test_teacher_rows(base, model, score):
    m = model
    base.makeup_score = m.makeup_score = score
    try:
        m.reset_conditioning_cache()
        batch = make_batch(m)
        log = m.log_results(batch, 0, seeds=5)
        base.reset_conditioning_cache()
        ref_log = base.log_results(make_batch(base), 0, seeds=5)
    finally:
        base.makeup_score = m.makeup_score = False
    assert set(log) == set(ref_log) | NEW | ({'makeup_hist_teacher'} if score else set())
    for k in ref_log:          # the rows that were there are the rows of a model without the teacher
        assert same(log[k], ref_log[k]), k
    dev = lambda k: batch[k].to(DEV)
    x_p = teacher.pseudo_ground_truth(dev('src_img'), dev('ref_img'), dev(m.seg_key), dev(m.ref_seg_key), feather=2)[0]
    assert same(log['ground_truth'], x_p * 2.0 - 1.0)
    sd = noise.as_seeds(5, 2)
    z = m.get_z(log['ground_truth'], seeds=sd)
    assert same(log['reconstruction'], m.decode_first_stage(z))
    t = torch.tensor(noise.teacher_timesteps(sd, 0, m.num_timesteps), device=DEV)
    nz = noise.normal(sd, (4, 8, 8), stream=noise.STREAM_TEACHER, device=DEV)
    x_noisy = m.sqrt_alphas_cumprod.to(DEV)[t].view(-1, 1, 1, 1) * z + m.sqrt_one_minus_alphas_cumprod.to(DEV)[t].view(-1, 1, 1, 1) * nz
    _, c = m.get_input(batch, m.first_stage_key)
    _, x0 = m.apply_model(x_noisy, t, {'c_concat': c['c_concat'], 'c_crossattn': c['c_crossattn']}, return_all=True)
    assert same(log['sample_ddmp'], m.decode_first_stage(x0))
    assert tuple(log['sample_ddmp'].shape) == (2, 3, 64, 64) and bool(torch.isfinite(log['sample_ddmp']).all())
    if score:
        assert same(log['makeup_hist_teacher'], m.makeup_hist(batch, log['ground_truth'], dev('ref_img')))
        assert tuple(log['makeup_hist_teacher'].shape) == (2, 4)


def test_teacher_rows_unseeded_draw_in_the_reference_order(model):
    """get_z's posterior noise (CPU generator), then torch.randint for t and torch.randn_like for the noise on the device"""
    m = model
    m.sample, scale, m.unconditional_guidance_scale = False, m.unconditional_guidance_scale, 1.0
    try:
        m.reset_conditioning_cache()
        batch = make_batch(m)
        torch.manual_seed(11)
        log = m.log_results(batch, 0)
        torch.manual_seed(11)
        z = m.get_z(log['ground_truth'])
        t = torch.randint(0, m.num_timesteps, (2,), device=DEV).long()
        nz = torch.randn_like(z)
    finally:
        m.sample, m.unconditional_guidance_scale = True, scale
    assert sorted(log) == ['control_ref', 'control_src', 'ground_truth', 'reconstruction', 'sample_ddmp']
    x_noisy = m.sqrt_alphas_cumprod.to(DEV)[t].view(-1, 1, 1, 1) * z + m.sqrt_one_minus_alphas_cumprod.to(DEV)[t].view(-1, 1, 1, 1) * nz
    _, c = m.get_input(batch, m.first_stage_key)
    _, x0 = m.apply_model(x_noisy, t, {'c_concat': c['c_concat'], 'c_crossattn': c['c_crossattn']}, return_all=True)
    assert same(log['reconstruction'], m.decode_first_stage(z)) and same(log['sample_ddmp'], m.decode_first_stage(x0))


def by_hand(m, batch, gt, sd, scale):
    """get_z -> stochastic_encode(k - 1) -> decode(k) from the existing calls"""
    solver, cls, options = m._sampler()
    smp = cls(m)
    if solver.name == 'ddim':
        smp.make_schedule(ddim_num_steps=STEPS, ddim_eta=0.0, verbose=False)
        ddim = smp
    else:
        smp.make_schedule(STEPS)
        ddim = DDIMSampler(m)
        ddim.make_schedule(ddim_num_steps=STEPS, ddim_eta=0.0, verbose=False)
    z = m.get_z(gt, seeds=sd)
    x = ddim.stochastic_encode(z, K - 1, seeds=sd)
    _, c = m.get_input(batch, m.first_stage_key)
    cond = {'c_concat': c['c_concat'], 'c_crossattn': c['c_crossattn']}
    uc = None if scale == 1.0 else {'c_concat': c['c_concat'], 'c_crossattn': [m.get_unconditional_conditioning(2)]}
    return smp.decode(x, cond, K, unconditional_guidance_scale=scale, unconditional_conditioning=uc, **options)


@pytest.mark.parametrize('scale', [1.0, 9.0])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp', 'unipc'])
def test_teacher_start_is_the_composition_and_runs_k_evaluations(model, sampler, scale):
    m = model
    m.sampler, m.unconditional_guidance_scale, m.teacher_start = sampler, scale, TAU
    try:
        assert teacher.start_steps(TAU, STEPS) == K
        sd = noise.as_seeds(21, 2)
        m.reset_conditioning_cache()
        with Evaluations(m) as ev:
            log = m.log_results(make_batch(m), 0, seeds=sd)
        passes = 1 if scale == 1.0 else 2
        assert ev.calls == [(sampler, K)] * passes, ev.calls                                        # k evaluations, not STEPS
        m.reset_conditioning_cache()
        again = m.log_results(make_batch(m), 0, seeds=sd)
        for key in log:
            assert same(log[key], again[key]), key                                                  # a seeded call repeats bit for bit
        m.reset_conditioning_cache()
        want = by_hand(m, make_batch(m), log['ground_truth'], sd, scale)
        name = 'samples_latent' if scale == 1.0 else f'samples_cfg_scale_{scale:.2f}_latent'
        assert same(log[name], want)
        assert same(log[name[:-7]], m.decode_first_stage(want))
        if scale != 1.0:
            m.reset_conditioning_cache()
            assert same(log['samples_latent'], by_hand(m, make_batch(m), log['ground_truth'], sd, 1.0))
        # tau = 1: all S evaluations, from the teacher latent diffused to the schedule's last entry
        m.teacher_start = 1.0
        m.reset_conditioning_cache()
        with Evaluations(m) as ev:
            full = m.log_results(make_batch(m), 0, seeds=sd)
        assert ev.calls == [(sampler, STEPS)] * passes and not same(full[name], log[name])
        # a pair's result does not depend on its place in the batch (equal batch sizes; bf16 kernels: the suite's per-kernel bound)
        m.teacher_start = TAU
        m.reset_conditioning_cache()
        swapped = m.log_results(make_batch(m, (1, 0)), 0, seeds=sd.take([1, 0]))
        assert same(swapped['ground_truth'], log['ground_truth'].flip(0))
        print(f'{sampler} scale {scale}: swapped batch bit-equal: {same(swapped[name], log[name].flip(0))}')
        assert_close_bf16(swapped[name], log[name].flip(0), what='swapped batch')
    finally:
        m.sampler, m.unconditional_guidance_scale, m.teacher_start = 'ddim', 9, None


def test_teacher_start_unseeded_takes_one_device_draw(model):
    m = model
    m.teacher_start, m.unconditional_guidance_scale = TAU, 9
    try:
        m.reset_conditioning_cache()
        torch.manual_seed(4)
        log = m.log_results(make_batch(m), 0)
        torch.manual_seed(4)
        z = m.get_z(log['ground_truth'])
        torch.randint(0, m.num_timesteps, (2,), device=DEV)
        torch.randn_like(z)                                                                          # (the sample_ddmp row's draws)
        smp = DDIMSampler(m)
        smp.make_schedule(ddim_num_steps=STEPS, ddim_eta=0.0, verbose=False)
        x = smp.stochastic_encode(z, K - 1)
        _, c = m.get_input(make_batch(m), m.first_stage_key)
        want = smp.decode(x, {'c_concat': c['c_concat'], 'c_crossattn': c['c_crossattn']}, K)
    finally:
        m.teacher_start = None
    assert same(log['samples_latent'], want)


def test_refused_combinations_raise_before_any_launch(model):
    m = model
    m.teacher_start = TAU
    try:
        for attr, val, back in (('fix_background', True, False), ('denoise_rows', True, False), ('guidance_rescale', 0.5, 0.0), ('ddim_eta', 0.5, 0.0)):
            setattr(m, attr, val)
            try:
                with DeviceCalls(m) as dc, pytest.raises(ValueError, match=attr):
                    m.log_results(make_batch(m), 0, seeds=1)
                assert not dc.calls, dc.calls          # nothing reached the engine or a libmkd wrapper
            finally:
                setattr(m, attr, back)
        frame = torch.zeros(64, 64, 3, dtype=torch.uint8)
        b = make_batch(m)
        del b[m.ref_seg_key]
        for word, call in (('x_T', lambda: m.log_results(make_batch(m), 0, x_T=torch.zeros(2, 4, 8, 8))),
                           ('transfer_specs', lambda: m.transfer_specs(make_batch(m), [])),
                           ('video', lambda: m.video_session(frame)),
                           ('video', lambda: m.transfer_video([frame, frame], frame)),
                           ('interpolate', lambda: m.interpolate(make_batch(m), [0.0, 1.0])),
                           ('transfer_regions', lambda: m.transfer_regions(make_batch(m), {'lip': 'ref_img'})),
                           ('label maps', lambda: m.log_results(b, 0))):
            with DeviceCalls(m) as dc, pytest.raises(ValueError, match=word):
                call()
            assert not dc.calls, (word, dc.calls)
    finally:
        m.teacher_start = None


# ---- transfer_photos(teacher_start=) ------------------------------------------------------------------------------------------------
def photos():
    """two source photos (one face each, a box of its own) and their references, with label maps at photo resolution: the synthetic
    faces scaled up by pixel repetition inside a noisy photo"""
    src, ref, ss, rs = tr.synthetic_pairs(n=2, size=32)
    g = torch.Generator().manual_seed(12)
    out = dict(src=[], ref=[], ssegs=[], rsegs=[], sboxes=[], rboxes=[])
    for i, ((H, W), (x0, y0)) in enumerate((((150, 203), (30, 10)), ((140, 160), (8, 5)))):
        for imgs, segs, kp, ks, kb in ((src, ss, 'src', 'ssegs', 'sboxes'), (ref, rs, 'ref', 'rsegs', 'rboxes')):
            p = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
            s = torch.zeros(H, W, dtype=torch.uint8)
            face = torch.from_numpy((imgs[i].transpose(1, 2, 0) * 255).astype(np.uint8)).repeat_interleave(4, 0).repeat_interleave(4, 1)
            p[y0:y0 + 128, x0:x0 + 128] = face
            s[y0:y0 + 128, x0:x0 + 128] = torch.from_numpy(segs[i]).repeat_interleave(4, 0).repeat_interleave(4, 1)
            out[kp].append(p), out[ks].append(s), out[kb].append((x0, y0, 128, 128))
    out['batch'] = {'txt_emb': torch.randn(2, 77, 64, generator=g)}
    return out


def test_transfer_photos_teacher_start(base, model):
    d = photos()
    m = model
    kw = dict(src_segs=d['ssegs'], feather=3, size=64, batch=d['batch'], seeds=40)
    m.reset_conditioning_cache()
    with Evaluations(m) as ev:
        got = m.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], ref_segs=d['rsegs'], teacher_start=TAU, **kw)
    assert ev.calls == [('ddim', K)]
    assert len(got) == 2
    for g, p, (x0, y0, bw, bh) in zip(got, d['src'], d['sboxes']):
        assert g.dtype == torch.uint8 and tuple(g.shape) == tuple(p.shape)
        g, p = g.cpu().numpy(), p.numpy()
        inside = np.zeros(p.shape[:2], bool)
        inside[y0:y0 + bh, x0:x0 + bw] = True
        assert np.array_equal(g[~inside], p[~inside]) and (g[inside] != p[inside]).mean() > 0.3
    m.reset_conditioning_cache()
    again = m.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], ref_segs=d['rsegs'], teacher_start=TAU, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # two faces in one photo, and a photo without a face: it comes back unchanged
    two = [[d['sboxes'][0], (140, 100, 50, 50)], []]
    m.reset_conditioning_cache()
    with Evaluations(m) as ev:
        many = m.transfer_photos(d['src'], d['ref'], two, d['rboxes'], ref_segs=d['rsegs'], teacher_start=TAU, max_faces=2, **kw)
    assert ev.calls == [('ddim', K)] and tuple(many[0].shape) == tuple(d['src'][0].shape)
    assert torch.equal(many[1].cpu(), d['src'][1])
    changed = (many[0].cpu() != d['src'][0]).any(-1)
    assert bool(changed[100:150, 140:190].any()) and bool(changed[10:138, 30:158].any()) and not bool(changed[140:, :30].any())
    # without the keyword the call is the call of a model built without the teacher keywords
    m.reset_conditioning_cache()
    base.reset_conditioning_cache()
    a = m.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], **kw)
    b = base.transfer_photos(d['src'], d['ref'], d['sboxes'], d['rboxes'], **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not any(torch.equal(x, y) for x, y in zip(a, got))
