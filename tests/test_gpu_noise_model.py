"""-m gpu: per-sample seeds through the samplers, the model and runs/test.py on the small engine of tests/test_gpu_unipc.py (B = 2, 8 x 8
latents, 10 steps).  A seeded call repeats bit for bit whatever the torch generators hold and leaves them alone; the tensors handed to
the engine are noise.normal of the documented stream and row and do not depend on the batch; a face of a photo draws from (the photo's
seed, its rank) whatever face_batch is; runs/test.py --device-noise writes the same bytes twice; and a call without seeds still draws
from the torch generators in the documented order."""
import os
import subprocess
import sys

import pytest
import torch

import vae_encoder_ref as enc_ref
from gpu_util import DEV
from makeupdiffuse_amd import noise
from makeupdiffuse_amd.batching import SampleSpec
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler
from makeupdiffuse_amd.unipc import UniPCSampler
from oracle import nets, vae

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))
S, B, SHAPE = 10, 2, (4, 8, 8)
SEEDS = [7, 9]


@pytest.fixture(scope='module')
def model():
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True,
                         ddim_steps=S, unconditional_guidance_scale=9)
    m.load_state_dict({**nets.init_state_dict(OCFG, seed=31), **vae.init_state_dict(vcfg, seed=32), **enc_ref.init_state_dict(vcfg, seed=33)})
    m.cuda(0)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(34))
    m.save_images = False
    return m


@pytest.fixture(scope='module')
def I():
    g = torch.Generator().manual_seed(35)
    return dict(hint=torch.rand(B, 6, 64, 64, generator=g).to(DEV), ctx=torch.randn(B, 77, 64, generator=g).to(DEV),
                x0=torch.randn(B, *SHAPE, generator=g).to(DEV), mask=(torch.rand(B, 1, 8, 8, generator=g) > 0.5).float().to(DEV),
                x_T=torch.randn(B, *SHAPE, generator=g).to(DEV))


def cond_of(I, sl=slice(None)):
    return {'c_crossattn': [I['ctx'][sl].contiguous()], 'c_concat': [I['hint'][sl].contiguous()]}


class Capture:
    """wraps the engine's sample entries (and the encoder) and keeps the tensors handed to them"""

    def __init__(self, monkeypatch, eng):
        self.calls, self.encodes = [], []
        for name in ('sample', 'sample_dpmpp', 'sample_unipc', 'sample_rows'):
            monkeypatch.setattr(eng, name, self._wrap(name, getattr(eng, name)))
        enc = eng.encode

        def encode(images, scale_factor=0.18215, noise=None, moments=False):
            self.encodes.append(None if noise is None else noise.clone())
            return enc(images, scale_factor, noise, moments)
        monkeypatch.setattr(eng, 'encode', encode)

    def _wrap(self, name, fn):
        def inner(x_T, *a, **kw):
            self.calls.append(dict(entry=name, x_T=x_T.clone(), args=a, kw=dict(kw), fn=fn,
                                   noise=None if kw.get('noise') is None else kw['noise'].clone(),
                                   q_noise=None if kw.get('q_noise') is None else kw['q_noise'].clone()))
            return fn(x_T, *a, **kw)
        return inner


def runs(m, I):
    """the four seeded calls of the repeatability test, each -> a latent"""
    c = cond_of(I)
    masked = dict(mask=I['mask'], x0=I['x0'])
    specs = [SampleSpec(steps=10, eta=0.5), SampleSpec(steps=5, eta=1.0)]
    return {
        'masked ddim eta 0.5': lambda **kw: DDIMSampler(m).sample(S, B, SHAPE, c, eta=0.5, verbose=False, **masked, **kw)[0],
        'masked dpmpp': lambda **kw: DPMSolverSampler(m).sample(S, B, SHAPE, c, order=2, **masked, **kw)[0],
        'unipc': lambda **kw: UniPCSampler(m).sample(S, B, SHAPE, c, order=2, **kw)[0],
        'specs': lambda **kw: DDIMSampler(m).sample_specs(specs, SHAPE, c, **kw),
    }


def rng_states():
    return torch.get_rng_state(), torch.cuda.get_rng_state(DEV)


# ---- 1. repeatability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['masked ddim eta 0.5', 'masked dpmpp', 'unipc', 'specs'])
def test_seeded_calls_repeat_and_leave_the_generators_alone(model, I, name):
    run = runs(model, I)[name]
    outs = []
    for s in (1, 2):
        torch.manual_seed(1000 + s)
        before = rng_states()
        model.reset_conditioning_cache()
        outs.append(run(seeds=SEEDS))
        torch.cuda.synchronize()
        after = rng_states()
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), f'{name}: a torch generator was advanced'
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]), name
    assert not torch.equal(outs[0], run(seeds=[8, 9]))          # the seed matters
    # an int is a start seed: s, s + 1
    assert torch.equal(run(seeds=7), run(seeds=[7, 8]))


def test_log_results_with_seeds_repeats(model, I):
    m = model
    g = torch.Generator().manual_seed(70)
    batch = {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g),
             'txt_emb': torch.randn(B, 77, 64, generator=g), 'nonmakeup_seg': torch.randint(0, 14, (B, 64, 64), generator=g, dtype=torch.uint8)}
    m.fix_background, m.ddim_eta = True, 0.5
    try:
        logs = []
        for s in (1, 2):
            torch.manual_seed(2000 + s)
            before = rng_states()
            m.reset_conditioning_cache()
            logs.append(m.log_results(dict(batch), 0, seeds=SEEDS))
            torch.cuda.synchronize()
            after = rng_states()
            assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])          # the posterior sample included
        m.seed = 7                                                                                   # the model's default seed: 7, 8
        by_default = m.log_results(dict(batch), 0)
        explicit = m.log_results(dict(batch), 0, seeds=[7, 8])
    finally:
        m.fix_background, m.ddim_eta, m.seed = False, 0.0, None
    for k in ('samples_latent', 'samples_cfg_scale_9.00_latent', 'samples'):
        assert torch.equal(logs[0][k], logs[1][k]), k
        assert torch.equal(by_default[k], explicit[k]), k
    assert not torch.equal(by_default['samples_latent'], logs[0]['samples_latent'])


# ---- 2. what the engine is handed -----------------------------------------------------------------------------------------------------
def test_the_engine_gets_the_documented_streams_and_rows(model, I, monkeypatch):
    m = model
    cap = Capture(monkeypatch, m.engine)
    N = lambda seeds, stream, **kw: noise.normal(seeds, SHAPE, stream=stream, device=DEV, **kw)
    masked = dict(mask=I['mask'], x0=I['x0'])
    # masked DDIM, eta 0.5: x_T on stream 0, the eta rows on stream 1, the blend rows on stream 2, row = executed step
    DDIMSampler(m).sample(S, B, SHAPE, cond_of(I), eta=0.5, verbose=False, seeds=SEEDS, **masked)
    c = cap.calls[-1]
    assert c['entry'] == 'sample' and tuple(c['noise'].shape) == (S, B, *SHAPE) and tuple(c['q_noise'].shape) == (S, B, *SHAPE)
    assert torch.equal(c['x_T'], N(SEEDS, noise.STREAM_START))
    assert torch.equal(c['noise'], N(SEEDS, noise.STREAM_ETA, rows=S)) and torch.equal(c['q_noise'], N(SEEDS, noise.STREAM_BLEND, rows=S))
    for k in (0, 3, S - 1):
        assert torch.equal(c['noise'][k], N(SEEDS, noise.STREAM_ETA, row0=k)) and torch.equal(c['q_noise'][k], N(SEEDS, noise.STREAM_BLEND, row0=k))
    # sample 0 alone gets the same tensors
    one = slice(0, 1)
    DDIMSampler(m).sample(S, 1, SHAPE, cond_of(I, one), eta=0.5, verbose=False, seeds=SEEDS[:1], mask=I['mask'][one], x0=I['x0'][one])
    a = cap.calls[-1]
    for k in ('x_T', 'noise', 'q_noise'):
        assert torch.equal(a[k], c[k][:, one] if k != 'x_T' else c[k][one]), k
    # seeds together with x_T: x_T as given, the other draws seeded
    DDIMSampler(m).sample(S, B, SHAPE, cond_of(I), eta=0.5, verbose=False, seeds=SEEDS, x_T=I['x_T'], **masked)
    g = cap.calls[-1]
    assert torch.equal(g['x_T'], I['x_T']) and torch.equal(g['noise'], c['noise']) and torch.equal(g['q_noise'], c['q_noise'])
    # the step-by-step loop (a callback) hands its hooks the same rows, one draw per step
    eta_rows, blend_rows = [], []
    step, blend = m.ddim_step, m.q_sample_blend
    monkeypatch.setattr(m, 'ddim_step', lambda *a, **kw: (eta_rows.append(a[8]), step(*a, **kw))[1])
    monkeypatch.setattr(m, 'q_sample_blend', lambda *a, **kw: (blend_rows.append(a[1]), blend(*a, **kw))[1])
    n_calls = len(cap.calls)
    DDIMSampler(m).sample(S, B, SHAPE, cond_of(I), eta=0.5, verbose=False, seeds=SEEDS, callback=lambda i: None, **masked)
    assert len(cap.calls) == n_calls and len(eta_rows) == len(blend_rows) == S
    assert torch.equal(torch.stack(eta_rows), c['noise']) and torch.equal(torch.stack(blend_rows), c['q_noise'])
    blend_rows.clear()
    DPMSolverSampler(m).sample(S, B, SHAPE, cond_of(I), seeds=SEEDS, callback=lambda i: None, **masked)
    assert torch.equal(torch.stack(blend_rows), c['q_noise'])
    monkeypatch.setattr(m, 'ddim_step', step)
    monkeypatch.setattr(m, 'q_sample_blend', blend)
    # masked DPM-Solver++: x_T and the blend rows; UniPC: x_T
    DPMSolverSampler(m).sample(S, B, SHAPE, cond_of(I), seeds=SEEDS, **masked)
    d = cap.calls[-1]
    assert d['entry'] == 'sample_dpmpp' and torch.equal(d['x_T'], c['x_T']) and torch.equal(d['q_noise'], c['q_noise']) and d['noise'] is None
    DPMSolverSampler(m).sample(S, 1, SHAPE, cond_of(I, one), seeds=SEEDS[:1], mask=I['mask'][one], x0=I['x0'][one])
    assert torch.equal(cap.calls[-1]['q_noise'], c['q_noise'][:, one]) and torch.equal(cap.calls[-1]['x_T'], c['x_T'][one])
    UniPCSampler(m).sample(S, B, SHAPE, cond_of(I), seeds=SEEDS)
    u = cap.calls[-1]
    assert u['entry'] == 'sample_unipc' and torch.equal(u['x_T'], c['x_T']) and u['noise'] is None and u['q_noise'] is None
    UniPCSampler(m).sample(S, 1, SHAPE, cond_of(I, slice(1, 2)), seeds=SEEDS[1:])
    assert torch.equal(cap.calls[-1]['x_T'], c['x_T'][1:2])
    # stochastic_encode: stream 2, row 0
    smp = DDIMSampler(m)
    smp.make_schedule(S, ddim_eta=0.0, verbose=False)
    enc = smp.stochastic_encode(I['x0'], [3, 3], seeds=SEEDS)
    assert torch.equal(enc, smp.stochastic_encode(I['x0'], [3, 3], noise=N(SEEDS, noise.STREAM_BLEND)))


def test_sample_specs_rows_are_those_of_the_uniform_calls(model, I, monkeypatch):
    m = model
    cap = Capture(monkeypatch, m.engine)
    specs = [SampleSpec(steps=10, eta=0.5), SampleSpec(steps=5, eta=1.0)]
    DDIMSampler(m).sample_specs(specs, SHAPE, cond_of(I), seeds=SEEDS)
    sp = cap.calls[-1]
    assert sp['entry'] == 'sample_rows' and tuple(sp['noise'].shape) == (10, B, *SHAPE)
    for b, spec in enumerate(specs):
        one = slice(b, b + 1)
        DDIMSampler(m).sample(spec.steps, 1, SHAPE, cond_of(I, one), eta=spec.eta, verbose=False, seeds=[SEEDS[b]])
        u = cap.calls[-1]
        n_b = u['noise'].shape[0]
        assert n_b == spec.steps
        assert torch.equal(u['x_T'], sp['x_T'][one]) and torch.equal(u['noise'], sp['noise'][:n_b, one]), b
    # the DPM-Solver++ form draws x_T alone; the model passes each pass its members' seeds
    DPMSolverSampler(m).sample_specs([SampleSpec(steps=10), SampleSpec(steps=5, order=3)], SHAPE, cond_of(I), seeds=SEEDS)
    assert torch.equal(cap.calls[-1]['x_T'], sp['x_T']) and cap.calls[-1]['kw'].get('noise') is None
    g = torch.Generator().manual_seed(71)
    batch = {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g), 'txt_emb': torch.randn(B, 77, 64, generator=g)}
    n0 = len(cap.calls)
    m.transfer_specs(batch, [SampleSpec(steps=4, guidance=3.0), SampleSpec(steps=6)], seeds=SEEDS)
    passes = cap.calls[n0:]
    assert len(passes) == 2          # the unguided pair (index 1) first, then the guided one (index 0)
    assert torch.equal(passes[0]['x_T'], sp['x_T'][1:2]) and torch.equal(passes[1]['x_T'], sp['x_T'][0:1])


# ---- 3. the photo path ----------------------------------------------------------------------------------------------------------------
def test_a_face_draws_from_its_photos_seed_and_its_rank_whatever_face_batch_is(model, monkeypatch):
    m = model
    g = torch.Generator().manual_seed(72)
    photo = torch.randint(0, 256, (120, 200, 3), generator=g, dtype=torch.uint8)
    ref = torch.randint(0, 256, (90, 80, 3), generator=g, dtype=torch.uint8)
    boxes = [(10, 20, 80, 80), (110, 30, 72, 72)]
    seg = torch.zeros(120, 200, dtype=torch.uint8)
    for x0, y0, bw, bh in boxes:          # background 0 around a face (1) with hair (12) on top
        seg[y0 + bh // 8:y0 + bh // 4, x0 + bw // 4:x0 + 3 * bw // 4] = 12
        seg[y0 + bh // 4:y0 + 7 * bh // 8, x0 + bw // 4:x0 + 3 * bw // 4] = 1
    text = {'txt_emb': torch.randn(1, 77, 64, generator=g)}
    cap = Capture(monkeypatch, m.engine)
    m.fix_background, m.ddim_steps = True, 4
    try:
        got = {}
        for fb in (1, 4):
            n0, e0 = len(cap.calls), len(cap.encodes)
            torch.manual_seed(3000 + fb)
            before = rng_states()
            m.transfer_photos([photo], [ref], [boxes], [(5, 5, 70, 70)], src_segs=[seg], size=64, batch=text, max_faces=2, face_batch=fb, seeds=[21])
            torch.cuda.synchronize()
            after = rng_states()
            assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
            calls, encs = cap.calls[n0:], cap.encodes[e0:]
            assert len(calls) == len(encs) == (2 if fb == 1 else 1)
            got[fb] = (torch.cat([c['x_T'] for c in calls]), torch.cat([c['q_noise'] for c in calls], dim=1), torch.cat(encs))
    finally:
        m.fix_background, m.ddim_steps = False, S
    for a, b in zip(got[1], got[4]):
        assert torch.equal(a, b)
    x_T, q, post = got[4]
    n = q.shape[0]
    for k in range(2):          # face k: the photo's seed, sub-stream k
        kw = dict(subs=[k], device=DEV)
        assert torch.equal(x_T[k:k + 1], noise.normal([21], SHAPE, stream=noise.STREAM_START, **kw))
        assert torch.equal(q[:, k:k + 1], noise.normal([21], SHAPE, stream=noise.STREAM_BLEND, rows=n, **kw))
        assert torch.equal(post[k:k + 1], noise.normal([21], SHAPE, stream=noise.STREAM_POSTERIOR, **kw))
    assert not torch.equal(x_T[0], x_T[1])


# ---- 4. runs/test.py --device-noise ---------------------------------------------------------------------------------------------------
def test_runs_test_py_with_device_noise_writes_the_same_bytes_twice(tmp_path):
    files = []
    for run in ('a', 'b'):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--pairs', '2', '--batch-size', '2', '--res', '64',
                            '--ddim-steps', '4', '--seed', '3', '--device-noise', '--fix-background', '--out', str(out)],
                           capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        root = out / 'makeupdiffuse_mi355x'
        files.append({n: (root / n).read_bytes() for n in sorted(os.listdir(root)) if n.endswith('.png')})
    assert sorted(files[0]) == sorted(files[1]) and 'samples_0000.png' in files[0] and 'samples_cfg_scale_9.00_0000.png' in files[0]
    for n in files[0]:
        assert files[0][n] == files[1][n], f'{n} differs between two runs of the same command'


# ---- 5. no seeds: the torch draws, in the documented order ----------------------------------------------------------------------------
def test_without_seeds_the_call_draws_from_the_torch_generators_as_before(model, I, monkeypatch):
    m = model
    cap = Capture(monkeypatch, m.engine)
    masked = dict(mask=I['mask'], x0=I['x0'])
    torch.manual_seed(4242)
    m.reset_conditioning_cache()
    out, _ = DDIMSampler(m).sample(S, B, SHAPE, cond_of(I), eta=0.5, verbose=False, **masked)
    c = cap.calls[-1]
    # the recorded torch.randn-driven call: x_T, then per executed step the blend's draw BEFORE the eta draw (every sigma is non-zero here)
    torch.manual_seed(4242)
    x_T = torch.randn((B, *SHAPE), device=DEV)
    q_rows, e_rows = [], []
    for _ in range(S):
        q_rows.append(torch.randn_like(I['x0']))
        e_rows.append(torch.randn((B, *SHAPE), device=DEV))
    assert torch.equal(c['x_T'], x_T) and torch.equal(c['q_noise'], torch.stack(q_rows)) and torch.equal(c['noise'], torch.stack(e_rows))
    kw = dict(c['kw'], noise=torch.stack(e_rows), q_noise=torch.stack(q_rows))
    m.reset_conditioning_cache()
    m._bind_guided(cond_of(I), None, 1.0, SHAPE[1:])
    res = c['fn'](x_T, *c['args'], **kw)
    res = res[0] if isinstance(res, tuple) else res
    assert torch.equal(res, out)
    # ... and the generators moved on: a second unseeded call differs, the same manual_seed repeats it
    torch.manual_seed(4242)
    again, _ = DDIMSampler(m).sample(S, B, SHAPE, cond_of(I), eta=0.5, verbose=False, **masked)
    other, _ = DDIMSampler(m).sample(S, B, SHAPE, cond_of(I), eta=0.5, verbose=False, **masked)
    assert torch.equal(again, out) and not torch.equal(other, out)
