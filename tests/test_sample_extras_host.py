"""CPU: the sampling loop's extras on the host side.  The log-row rule against the step loop's appended indices and the library's
mkd_sample_log_rows, the samplers' intermediates from a trace-keeping fast hook against the step loop, guidance rescale against the
float64 restatement, and the model plumbing (TestDiffuseModel denoise_rows / log_every_t / guidance_rescale) on a recording engine."""
import os

import numpy as np
import pytest
import torch

import dpm_solver_ref as dref
import sample_extras_ref as xref
from makeupdiffuse_amd.config import create_model
from makeupdiffuse_amd.ddim import DDIMSampler, rescale_guided_eps
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler
from makeupdiffuse_amd.engine import sample_log_rows
from oracle import sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_ALL = (1, 3, 7, 10, 50)
L_ALL = (1, 3, 10, 100)


class HostModel:
    """Stand-in model on the host: schedule tables + an eps function; no device hooks."""

    def __init__(self, eps_fn, T=1000):
        sch = sampler.Schedule(timesteps=T)
        self.num_timesteps = T
        self.alphas_cumprod = sch.alphas_cumprod
        self.alphas_cumprod_prev = sch.alphas_cumprod_prev
        self.betas = torch.tensor(np.diff(np.append(0.0, 1.0 - sch.alphas_cumprod64)), dtype=torch.float32)
        self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(sch.alphas_cumprod64), dtype=torch.float32)
        self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - sch.alphas_cumprod64), dtype=torch.float32)
        self.device = torch.device('cpu')
        self.eps_fn = eps_fn

    def apply_model(self, x, t, c):
        return self.eps_fn(x, t, c)


def eps_cond(x, t, c):
    """an eps that depends on x, the timestep and the conditioning, with another spread per sample (the rescale factors differ)"""
    w = torch.linspace(0.5, 2.0, x.shape[0]).view(-1, 1, 1, 1)
    return 0.3 * torch.tanh(x) * w + 0.05 * c['v'] * torch.sin(x * 3.0 + t.view(-1, 1, 1, 1).float() * 0.01)


def conds(B):
    return {'v': torch.full((B, 1, 1, 1), 2.0)}, {'v': torch.full((B, 1, 1, 1), -1.0)}


def ref_cond(c):
    """the restated loops batch dict-of-lists conditionings"""
    return {'v': [c['v']]}


def ref_eps(x, t, c):
    return eps_cond(x, t, {'v': c['v'][0]})


# ---- 1. the row rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', S_ALL)
def test_row_rule_equals_the_step_loops_appended_indices(S):
    """what the step loop of DDIMSampler / DPMSolverSampler appends (a callback forces it) is the rule's entries, in its order"""
    m = HostModel(lambda x, t, c: 0.1 * x)
    x_T = torch.randn(1, 4, 2, 2)
    for L in L_ALL:
        entries = xref.logged_entries(S, L)
        # DDIMSampler: exactly S steps as the first S entries of a 50-entry schedule (the uniform grid has no 3- or 7-entry form)
        smp, seen = DDIMSampler(m), []
        smp.make_schedule(50, verbose=False)
        out, inter = smp.ddim_sampling({}, (1, 4, 2, 2), x_T=x_T, callback=seen.append, log_every_t=L, timesteps=smp.ddim_timesteps[:S])
        assert seen == list(range(S))
        assert len(inter['x_inter']) == len(inter['pred_x0']) == 1 + len(entries)
        assert inter['x_inter'][0] is x_T and inter['pred_x0'][0] is x_T and inter['x_inter'][-1] is out
        # which steps were appended: replay the loop and compare every appended latent with the latent after that executed step
        after = smp.ddim_sampling({}, (1, 4, 2, 2), x_T=x_T, callback=lambda i: None, log_every_t=1,
                                  timesteps=smp.ddim_timesteps[:S])[1]['x_inter'][1:]
        assert len(after) == S
        for row, i in zip(inter['x_inter'][1:], entries):
            assert torch.equal(row, after[S - 1 - i])
        if 1000 % S == 0:            # DPMSolverSampler.sample builds its own grid
            dpm, seen = DPMSolverSampler(m), []
            out, inter = dpm.sample(S, 1, (4, 2, 2), x_T=x_T, log_every_t=L, callback=seen.append)
            assert seen == list(range(S)) and len(dpm.ddim_timesteps) == S
            assert len(inter['x_inter']) == len(inter['pred_x0']) == 1 + len(entries)
            assert inter['x_inter'][0] is x_T and inter['pred_x0'][0] is x_T and inter['x_inter'][-1] is out
            after = dpm.sample(S, 1, (4, 2, 2), x_T=x_T, log_every_t=1, callback=lambda k: None)[1]['x_inter'][1:]
            for row, i in zip(inter['x_inter'][1:], entries):
                assert torch.equal(row, after[S - 1 - i])
        # the grid-free statement of the rule, for exactly S entries
        e = xref.logged_entries(S, L)
        assert e[0] == S - 1 and e[-1] == 0 and e == sorted(set(e), reverse=True)
        assert set(e) == {i for i in range(S) if i % L == 0} | {S - 1}


@pytest.mark.parametrize('S', S_ALL)
@pytest.mark.parametrize('L', L_ALL)
def test_library_row_count_equals_the_rule(S, L):
    assert sample_log_rows(S, L) == len(xref.logged_entries(S, L))


def test_library_row_count_rejects_bad_arguments():
    for bad in ((0, 1), (5, 0), (-1, 3), (5, -2)):
        with pytest.raises(ValueError):
            sample_log_rows(*bad)


# ---- 2. the samplers' lists: a trace-keeping fast hook against the step loop -------------------------------------------------------
@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('L', [1, 3, 100])
def test_ddim_fast_path_lists_equal_the_step_loops(guided, L):
    B, S = 2, 10
    c, uc = conds(B)
    x_T = torch.randn(B, 4, 3, 3, generator=torch.Generator().manual_seed(1))
    scale = 4.0 if guided else 1.0
    kw = dict(conditioning=c, x_T=x_T, eta=0.0, verbose=False, log_every_t=L, unconditional_guidance_scale=scale,
              unconditional_conditioning=uc if guided else None)
    m = HostModel(eps_cond)
    steps_out, steps = DDIMSampler(m).sample(S, B, (4, 3, 3), callback=lambda i: None, **kw)
    seen = {}

    def fast(x, cond, timesteps, alphas, alphas_prev, s1m, scale_=1.0, uc_=None, **k):
        """the in-library loop's contract: (latent, x_inter rows, pred_x0 rows) stacked, for the log_every_t it is handed"""
        seen.update(k)
        sch = sampler.Schedule().make_ddim(S)
        img, xs, x0s = xref.ddim_loop(ref_eps, sch, x, ref_cond(cond), scale_, None if uc_ is None else ref_cond(uc_), log_every_t=k['log_every_t'])
        return img, torch.stack(xs), torch.stack(x0s)
    m.sample_loop_fast = fast
    fast_out, lists = DDIMSampler(m).sample(S, B, (4, 3, 3), **kw)
    assert seen['log_every_t'] == L and 'guidance_rescale' not in seen
    for key in ('x_inter', 'pred_x0'):
        assert len(lists[key]) == len(steps[key]) == 1 + sample_log_rows(S, L), key
        assert lists[key][0] is x_T
        for a, b in zip(lists[key][1:], steps[key][1:]):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    assert lists['x_inter'][-1] is fast_out                       # the returned latent stays the last x_inter entry
    torch.testing.assert_close(fast_out, steps_out, rtol=1e-5, atol=1e-5)
    assert (lists['pred_x0'][-1] - x_T).abs().max() > 1e-2           # (the last x0-prediction is no longer the start noise)
    # a hook that keeps no trace (returns the latent alone) still gives the two-entry list
    m.sample_loop_fast = lambda x, *a, **k: x + 1.0
    out, lists = DDIMSampler(m).sample(S, B, (4, 3, 3), **kw)
    assert len(lists['x_inter']) == 2 and lists['x_inter'][-1] is out and len(lists['pred_x0']) == 1


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('L', [1, 3, 100])
def test_dpm_fast_path_lists_equal_the_step_loops(order, L):
    B, S = 2, 10
    c, uc = conds(B)
    x_T = torch.randn(B, 4, 3, 3, generator=torch.Generator().manual_seed(2))
    kw = dict(conditioning=c, x_T=x_T, order=order, log_every_t=L, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    m = HostModel(eps_cond)
    steps_out, steps = DPMSolverSampler(m).sample(S, B, (4, 3, 3), callback=lambda i: None, **kw)

    def fast(x, cond, timesteps, alphas, alphas_prev, order_, lof, scale_=1.0, uc_=None, **k):
        img, xs, x0s = xref.dpm_loop(ref_eps, timesteps, alphas, alphas_prev, x, ref_cond(cond), order_, lof, scale_, ref_cond(uc_),
                                     log_every_t=k['log_every_t'])
        return img, torch.stack(xs), torch.stack(x0s)
    m.sample_loop_dpmpp = fast
    fast_out, lists = DPMSolverSampler(m).sample(S, B, (4, 3, 3), **kw)
    for key in ('x_inter', 'pred_x0'):
        assert len(lists[key]) == len(steps[key]) == 1 + sample_log_rows(S, L), key
        for a, b in zip(lists[key][1:], steps[key][1:]):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    assert lists['x_inter'][0] is x_T and lists['x_inter'][-1] is fast_out


# ---- 3. guidance rescale ------------------------------------------------------------------------------------------------------------
def test_rescale_formula_against_float64():
    g = torch.Generator().manual_seed(3)
    B = 3
    e_c = torch.randn(B, 4, 5, 5, generator=g) * torch.tensor([1.0, 1e-3, 50.0]).view(B, 1, 1, 1)
    e_u = torch.randn(B, 4, 5, 5, generator=g)
    for phi in (0.3, 0.7, 1.0):
        k = xref.rescale_factor64(e_c, e_u, 9.0, phi)
        gd = e_u.double() + 9.0 * (e_c.double() - e_u.double())
        for b in range(B):            # the definition, written out per sample
            want = phi * e_c[b].double().std(unbiased=True) / gd[b].std(unbiased=True) + (1.0 - phi)
            assert abs(float(k[b]) - float(want)) <= 1e-12 * abs(float(want))
        assert len({round(float(v), 6) for v in k}) == B            # per sample, not one factor for the batch
        got = rescale_guided_eps(e_c, e_u, 9.0, phi)
        torch.testing.assert_close(got.double(), gd * k.view(B, 1, 1, 1), rtol=2e-5, atol=1e-6)
    # phi = 1: the rescaled eps has the conditional eps' per-sample std
    out = xref.rescaled_eps(e_c.double(), e_u.double(), 9.0, 1.0)
    torch.testing.assert_close(out.reshape(B, -1).std(dim=1), e_c.double().reshape(B, -1).std(dim=1), rtol=1e-10, atol=0)
    # std(g) == 0 gives k = 1 and stays finite
    const = torch.full((1, 4, 2, 2), 0.3)
    assert float(xref.rescale_factor64(const, const, 9.0, 0.7)) == 1.0
    assert torch.equal(rescale_guided_eps(const, const, 9.0, 0.7), const)


@pytest.mark.parametrize('which', ['ddim', 'ddim_eta', 'ddim_masked', 'dpm2', 'dpm3'])
@pytest.mark.parametrize('phi', [0.3, 0.7, 1.0])
def test_samplers_rescale_against_the_restatement(which, phi):
    B, S, scale = 2, 10, 9.0
    c, uc = conds(B)
    g = torch.Generator().manual_seed(4)
    # float64 latents: the samplers' coefficient form and the restatement's difference-quotient form then agree to the fp32 tables
    x_T, x0 = torch.randn(B, 4, 3, 3, generator=g).double(), torch.randn(B, 4, 3, 3, generator=g).double()
    mask = (torch.rand(B, 1, 3, 3, generator=g) > 0.5).double()
    m = HostModel(eps_cond)
    kw = dict(conditioning=c, x_T=x_T, unconditional_guidance_scale=scale, unconditional_conditioning=uc, log_every_t=3)
    factors = []
    if which.startswith('ddim'):
        eta = 0.5 if which == 'ddim_eta' else 0.0
        mk = dict(mask=mask, x0=x0) if which == 'ddim_masked' else {}
        run = lambda **k: DDIMSampler(m).sample(S, B, (4, 3, 3), eta=eta, verbose=False, **kw, **mk, **k)
        torch.manual_seed(40)
        out, inter = run(guidance_rescale=phi)
        sch = sampler.Schedule().make_ddim(S, eta)
        torch.manual_seed(40)
        q_draws, eta_draws = [], []
        for i in range(S):                                    # the step loop's draws in its order: the blend's, then the eta draw
            if mk:
                q_draws.append(torch.randn_like(x0))
            eta_draws.append(torch.randn(x_T.shape) if float(sch.ddim_sigmas[S - 1 - i]) != 0.0 else None)
        ref, xs, x0s = xref.ddim_loop(ref_eps, sch, x_T, ref_cond(c), scale, ref_cond(uc), phi, 3, x0 if mk else None, mask if mk else None,
                                      q_draws, eta_draws, factors=factors)
    else:
        order = int(which[-1])
        run = lambda **k: DPMSolverSampler(m).sample(S, B, (4, 3, 3), order=order, **kw, **k)
        out, inter = run(guidance_rescale=phi)
        ts, a, ap = dref.grid(S)
        ref, xs, x0s = xref.dpm_loop(ref_eps, ts, a, ap, x_T, ref_cond(c), order, True, scale, ref_cond(uc), phi, 3, factors=factors)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    assert len(inter['pred_x0']) == 1 + len(x0s) == 1 + sample_log_rows(S, 3)
    for a_, b_ in zip(inter['pred_x0'][1:] + inter['x_inter'][1:], x0s + xs):
        torch.testing.assert_close(a_, b_, rtol=1e-5, atol=1e-5)
    ks = torch.stack(factors)
    assert len(factors) == S and (ks[:, 0] - ks[:, 1]).abs().max() > 1e-3          # per step, and the two samples' factors differ
    # the rescale moves the latent (not a vacuous comparison); phi = 0 is the plain call, exactly
    torch.manual_seed(40)
    plain, plain_inter = run()
    assert ((out - plain).norm() / plain.norm()).item() > 1e-2
    torch.manual_seed(40)
    zero, zero_inter = run(guidance_rescale=0.0)
    assert torch.equal(zero, plain)
    assert all(torch.equal(a_, b_) for key in ('x_inter', 'pred_x0') for a_, b_ in zip(zero_inter[key], plain_inter[key]))


def test_rescale_is_not_engaged_without_guidance_and_rejects_bad_phi():
    B, S = 2, 5
    c, uc = conds(B)
    x_T = torch.randn(B, 4, 3, 3)
    m = HostModel(eps_cond)
    seen = {}
    for smp, kw in ((DDIMSampler(m), dict(eta=0.0, verbose=False)), (DPMSolverSampler(m), {})):
        plain, _ = smp.sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, callback=lambda i: None, **kw)
        # no unconditional half, or scale 1: phi changes nothing
        a, _ = smp.sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, guidance_rescale=0.7, callback=lambda i: None, **kw)
        b, _ = smp.sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, guidance_rescale=0.7, unconditional_guidance_scale=1.0,
                          unconditional_conditioning=uc, callback=lambda i: None, **kw)
        assert torch.equal(a, plain) and torch.equal(b, plain)
        for bad in (-0.1, 1.5, float('nan')):
            with pytest.raises(ValueError):
                smp.sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, guidance_rescale=bad, **kw)
    with pytest.raises(ValueError):
        DPMSolverSampler(m).sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, log_every_t=0)
    with pytest.raises(ValueError):
        DDIMSampler(m).p_sample_ddim(x_T, c, torch.zeros(B, dtype=torch.long), 0, guidance_rescale=2.0)

    # the fast hooks get phi only when it is engaged
    def fast(x, *a, **k):
        seen.update(k)
        return x
    m.sample_loop_fast = fast
    m.sample_loop_dpmpp = fast
    for smp, kw in ((DDIMSampler(m), dict(eta=0.0, verbose=False)), (DPMSolverSampler(m), {})):
        seen.clear()
        smp.sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, guidance_rescale=0.7, **kw)
        assert 'guidance_rescale' not in seen
        smp.sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, guidance_rescale=0.7, unconditional_guidance_scale=9.0,
                   unconditional_conditioning=uc, **kw)
        assert seen['guidance_rescale'] == 0.7 and seen['log_every_t'] == 100
        seen.clear()
        smp.sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, guidance_rescale=0.0, unconditional_guidance_scale=9.0,
                   unconditional_conditioning=uc, **kw)
        assert 'guidance_rescale' not in seen


# ---- 4. model plumbing on a recording engine (the pattern of test_host_logic.py) ---------------------------------------------------
class _RecordingEngine:
    """Stands for MkdEngine on the CPU: records the sampling calls, answers them with tagged tensors and trace rows."""
    vae_cfg = object()

    def __init__(self):
        self.calls = []

    def prepare(self, hint, ctx, **kw):
        pass

    def _run(self, name, x_T, n, kw):
        self.calls.append((name, dict(kw)))
        out = x_T + 1.0
        if not kw.get('want_trace'):
            return out
        rows = sample_log_rows(n, kw['log_every_t'])
        xs = torch.stack([x_T + 10.0 * (r + 1) for r in range(rows)])
        return out, xs, xs + 0.5

    def sample(self, x_T, timesteps, alphas, alphas_prev, s1m, **kw):
        return self._run('sample', x_T, len(timesteps), kw)

    def sample_dpmpp(self, x_T, timesteps, alphas, alphas_prev, **kw):
        return self._run('sample_dpmpp', x_T, len(timesteps), kw)

    def decode(self, z, scale_factor):
        return z[:, :3].repeat_interleave(8, 2).repeat_interleave(8, 3) * 2.0


def recording_model(**attrs):
    m = create_model(os.path.join(ROOT, 'diffmodels', 'test_diffusion_makeup.yaml'))
    eng = _RecordingEngine()
    m._require_engine = lambda: eng
    m.engine = eng
    m.uncond_embedding = torch.zeros(1, 77, m.net_config.context_dim)
    m.save_images = False
    m.ddim_steps = 10
    for k, v in attrs.items():
        setattr(m, k, v)
    return m, eng


def small_batch(m, B=2):
    g = torch.Generator().manual_seed(5)
    return {'src_img': torch.rand(B, 3, 16, 16, generator=g), 'ref_img': torch.rand(B, 3, 16, 16, generator=g),
            'txt_emb': torch.randn(B, 77, m.net_config.context_dim, generator=g)}


@pytest.mark.parametrize('which', ['ddim', 'dpmpp'])
def test_log_results_denoise_rows_and_rescale_plumbing(which):
    m, eng = recording_model(sampler=which, denoise_rows=True, log_every_t=3, guidance_rescale=0.7)
    B = 2
    x_T = torch.randn(B, 4, 2, 2)
    log = m.log_results(small_batch(m, B), 0, x_T=x_T)
    name = 'sample' if which == 'ddim' else 'sample_dpmpp'
    assert [c[0] for c in eng.calls] == [name, name]
    plain, guided = eng.calls[0][1], eng.calls[1][1]
    assert plain['want_trace'] and plain['log_every_t'] == 3 and plain['guidance_rescale'] == 0.0 and plain['cfg_scale'] == 1.0
    assert guided['want_trace'] and guided['log_every_t'] == 3 and guided['guidance_rescale'] == 0.7 and guided['cfg_scale'] == 9.0
    n = 1 + sample_log_rows(10, 3)                                   # list entries: x_T, then the logged steps
    for key in ('denoise_row', 'denoise_row_cfg_scale_9.00'):
        lat, img = log[key + '_latent'], log[key]
        assert tuple(lat.shape) == (B * n, 4, 2, 2) and tuple(img.shape) == (B * n, 3, 16, 16)
        for b in range(B):                                            # 'b n': samples as rows, list entries as columns
            assert torch.equal(lat[b * n], x_T[b])
            for j in range(1, n):
                assert torch.equal(lat[b * n + j], x_T[b] + 10.0 * j + 0.5)
                assert torch.equal(img[b * n + j], eng.decode(lat[b * n + j][None], 1.0)[0])
    assert torch.equal(log['samples_latent'], x_T + 1.0)


def test_log_results_is_unchanged_without_the_options():
    m, eng = recording_model()
    log = m.log_results(small_batch(m), 0, x_T=torch.randn(2, 4, 2, 2))
    assert not [k for k in log if k.startswith('denoise_row')]
    assert sorted(log) == ['control_ref', 'control_src', 'samples', 'samples_cfg_scale_9.00', 'samples_cfg_scale_9.00_latent', 'samples_latent']
    assert all(c[1]['guidance_rescale'] == 0.0 for c in eng.calls)


def test_model_rejects_bad_settings():
    from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
    for bad in (dict(log_every_t=0), dict(guidance_rescale=1.5), dict(guidance_rescale=-0.1)):
        with pytest.raises(ValueError):
            TestDiffuseModel(**bad)                          # (checked before anything is built)
