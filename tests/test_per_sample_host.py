"""Per-sample requests in one batch, host side (no GPU): the table builder against the samplers' own tables, the step table and
its time-embedding row map, the draw-order rule, the Python layer's argument errors, and the float64 restatement of both per-sample
updates against a loop of the single-request restatements."""
import numpy as np
import pytest
import torch

import dpm_solver_ref as dref
import per_sample_ref as pref
from makeupdiffuse_amd import batching
from makeupdiffuse_amd.batching import RowTables, SampleSpec, build_rows, draw_noise, draw_plan, start_rows, step_map
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler
from makeupdiffuse_amd.engine import STEP_ROW_DTYPE, dpmpp_table, pack_sample_rows, step_table
from makeupdiffuse_amd.lib import MkdError
from makeupdiffuse_amd.schedule import DDIMSchedule
from oracle import sampler


class StandIn:
    """what a sampler needs of a model: the DDPM tables"""
    device = 'cpu'

    def __init__(self):
        sch = DDIMSchedule()
        self.num_timesteps = sch.num_timesteps
        for k in ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod'):
            setattr(self, k, getattr(sch, k))


SPECS = [SampleSpec(10), SampleSpec(7, eta=0.5, guidance=9.0), SampleSpec(4, eta=1.0, guidance=1.5), SampleSpec(50, t_start=20),
         SampleSpec(1), SampleSpec(500, eta=0.3)]


# ---- the table builder ---------------------------------------------------------------------------------------------------------
def test_ddim_rows_are_make_schedules_tables():
    m = StandIn()
    rows = build_rows(SPECS, m.alphas_cumprod)
    for sp, row in zip(SPECS, rows):
        smp = DDIMSampler(m)
        smp.make_schedule(sp.steps, ddim_eta=sp.eta, verbose=False)
        n = len(smp.ddim_timesteps) if sp.t_start is None else sp.t_start          # (S = 7 gives upstream's 8-entry grid: all of it runs)
        assert row.n == n and row.cfg_scale == sp.guidance
        assert np.array_equal(row.timesteps, smp.ddim_timesteps[:n])
        # what the uniform path hands to libmkd: float(v) of each entry, stored as float
        for name, ref in (('alphas', smp.ddim_alphas), ('alphas_prev', smp.ddim_alphas_prev), ('sqrt_one_minus_alphas', smp.ddim_sqrt_one_minus_alphas)):
            want = np.asarray([float(v) for v in ref[:n]], dtype=np.float32)
            got = getattr(row, name)
            assert got.dtype == np.float32 and np.array_equal(got, want), (sp, name)
        sig = np.asarray([float(v) for v in smp.ddim_sigmas[:n]], dtype=np.float32)
        if sp.eta == 0.0:
            assert row.sigmas is None and not sig.any()
        else:
            assert np.array_equal(row.sigmas, sig) and sig.any()
        assert row.dpm is None


def test_dpm_rows_are_dpmpp_tables_rows():
    m = StandIn()
    specs = [SampleSpec(10, order=2), SampleSpec(5, order=3, guidance=3.0), SampleSpec(8, order=1), SampleSpec(20, order=3, t_start=6)]
    rows = build_rows(specs, m.alphas_cumprod, solver='dpmpp')
    for sp, row in zip(specs, rows):
        smp = DPMSolverSampler(m)
        smp.make_schedule(sp.steps)
        n = len(smp.ddim_timesteps) if sp.t_start is None else sp.t_start
        a = [float(v) for v in smp.ddim_alphas[:n]]; ap = [float(v) for v in smp.ddim_alphas_prev[:n]]
        coef, orders = dpmpp_table(a, ap, sp.order, True)
        assert row.dpm.shape == (n, 6) and row.dpm.dtype == np.float32 and np.array_equal(row.dpm, coef)
        assert orders.max() == min(sp.order, n) and row.sigmas is None
        assert np.array_equal(row.timesteps, smp.ddim_timesteps[:n])
        c64, _ = dref.coefficients(a, ap, sp.order)          # ... which is the independent derivation's table, rounded to float
        assert np.allclose(row.dpm, c64, rtol=2e-6, atol=1e-7)
    with pytest.raises(ValueError, match='deterministic'):
        build_rows([SampleSpec(10, eta=0.5)], m.alphas_cumprod, solver='dpmpp')


def test_builder_leaves_a_samplers_buffers_alone():
    m = StandIn()
    smp = DDIMSampler(m)
    smp.make_schedule(20, ddim_eta=0.25, verbose=False)
    names = ('ddim_sigmas', 'ddim_alphas', 'ddim_sqrt_one_minus_alphas', 'alphas_cumprod', 'betas')
    before = {k: getattr(smp, k).clone() for k in names}
    ids = {k: id(getattr(smp, k)) for k in names}
    ts, ap = smp.ddim_timesteps.copy(), np.array(smp.ddim_alphas_prev)
    ac = m.alphas_cumprod.clone()

    class Model(StandIn):
        def sample_rows_fast(self, x, cond, rows, solver, uc, noise, temperature):
            return x, rows, noise
    mm = Model()
    s2 = DDIMSampler(mm)
    s2.make_schedule(20, ddim_eta=0.25, verbose=False)
    snap = {k: getattr(s2, k).clone() for k in names}
    s2.sample_specs([SampleSpec(7), SampleSpec(30, eta=1.0)], (4, 2, 2), None, x_T=torch.zeros(2, 4, 2, 2))
    s2.decode(torch.zeros(2, 4, 2, 2), None, [3, 20]) if not s2.ddim_sigmas.any() else None
    build_rows(SPECS, m.alphas_cumprod)
    for k in names:
        assert id(getattr(smp, k)) == ids[k] and torch.equal(getattr(smp, k), before[k])
        assert torch.equal(getattr(s2, k), snap[k]), k
    assert np.array_equal(smp.ddim_timesteps, ts) and np.array_equal(smp.ddim_alphas_prev, ap) and torch.equal(m.alphas_cumprod, ac)
    assert len(s2.ddim_timesteps) == 20


def test_start_rows_cut_one_schedule():
    m = StandIn()
    smp = DDIMSampler(m)
    smp.make_schedule(10, verbose=False)
    rows = start_rows(torch.tensor([6, 3, 10]), smp.ddim_timesteps, smp.ddim_alphas, smp.ddim_alphas_prev, smp.ddim_sqrt_one_minus_alphas, cfg_scale=9.0)
    for n, row in zip((6, 3, 10), rows):
        assert row.n == n and row.cfg_scale == 9.0 and row.sigmas is None
        assert np.array_equal(row.timesteps, smp.ddim_timesteps[:n])
        assert np.array_equal(row.alphas, np.asarray([float(v) for v in smp.ddim_alphas[:n]], dtype=np.float32))
        assert np.array_equal(row.alphas_prev, np.asarray(smp.ddim_alphas_prev[:n], dtype=np.float32))
    for bad in ([0, 3, 10], [6, 11, 1], []):
        with pytest.raises(ValueError):
            start_rows(bad, smp.ddim_timesteps, smp.ddim_alphas, smp.ddim_alphas_prev, smp.ddim_sqrt_one_minus_alphas)


# ---- the step table and its time-embedding row map -------------------------------------------------------------------------------
def test_step_table_entries_and_row_map():
    m = StandIn()
    specs = [SampleSpec(10, guidance=9.0), SampleSpec(7, eta=0.5), SampleSpec(4, eta=1.0, guidance=1.5), SampleSpec(10)]
    rows = build_rows(specs, m.alphas_cumprod)
    tab, distinct = step_table(rows)
    entry, active, temb, want_distinct = step_map(rows)
    assert tab.dtype == STEP_ROW_DTYPE and tab.shape == (10, 4)
    assert distinct == want_distinct and len(set(distinct)) == len(distinct)
    assert np.array_equal(tab['active'].astype(bool), active) and np.array_equal(tab['temb_row'], temb)
    # first-seen order, steps outer, samples inner: step 0 holds the four samples' first timesteps in batch order
    first = [int(r.timesteps[-1]) for r in rows]
    assert distinct[:len(dict.fromkeys(first))] == list(dict.fromkeys(first))
    for k in range(10):
        for b, row in enumerate(rows):
            e = tab[k, b]
            i = entry[k, b]
            assert e['t'] == row.timesteps[i] == distinct[e['temb_row']] and e['scale'] == np.float32(row.cfg_scale)
            if k >= row.n:          # finished: its entry 0, flagged
                assert not e['active'] and i == 0 and e['t'] == row.timesteps[0]
                continue
            assert e['active'] == 1 and i == row.n - 1 - k
            sg = np.float32(0.0) if row.sigmas is None else row.sigmas[i]
            one = np.float32(1.0)
            want = (one / np.sqrt(row.alphas[i]), np.sqrt(row.alphas_prev[i]), np.sqrt(one - row.alphas_prev[i] - sg * sg), row.sqrt_one_minus_alphas[i])
            assert e['sigma'] == sg and np.array_equal(e['coef'], np.asarray(want, dtype=np.float32)), (k, b)
    # two samples with the same request share their rows of the time-embedding table: 10-step rows 0 and 3
    assert np.array_equal(tab['temb_row'][:, 0], tab['temb_row'][:, 3])
    # DPM-Solver++: the six numbers of the sample's entry
    drows = build_rows([SampleSpec(10, order=2), SampleSpec(5, order=3), SampleSpec(8, order=1)], m.alphas_cumprod, solver='dpmpp')
    dtab, _ = step_table(drows, 'dpmpp')
    for k in range(10):
        for b, row in enumerate(drows):
            if k < row.n:
                assert dtab[k, b]['active'] and np.array_equal(dtab[k, b]['dpm'], row.dpm[row.n - 1 - k])
            else:
                assert not dtab[k, b]['active'] and dtab[k, b]['t'] == row.timesteps[0]


def test_step_table_refusals():
    m = StandIn()
    good = build_rows([SampleSpec(4), SampleSpec(2)], m.alphas_cumprod)
    r = lambda **kw: dict(timesteps=good[0].timesteps, alphas=good[0].alphas, alphas_prev=good[0].alphas_prev,
                          sqrt_one_minus_alphas=good[0].sqrt_one_minus_alphas, **kw)
    cases = [([r(n_steps=0)], 'n_steps must be >= 1'), ([r(), r(n_steps=1025)], 'sample 1: n_steps exceeds MKD_MAX_STEPS'),
             ([r(), dict(r(), alphas=None)], 'sample 1: null table'), ([dict(r(), timesteps=None, n_steps=4)], 'null timesteps'),
             ([r(), r(sigmas=[0.0, 0.0, 2.0, 0.0])], 'sample 1: sigma out of range'), ([r(sigmas=[0.0, -0.1, 0.0, 0.0])], 'sigma out of range'),
             ([r(sigmas=[float('nan')] * 4)], 'sigma out of range')]
    for rows, msg in cases:
        with pytest.raises(MkdError, match=msg):
            step_table(rows)
    with pytest.raises(MkdError, match='null table'):
        step_table([r()], 'dpmpp')
    # more distinct timesteps than the time-embedding table holds: three samples of 600 steps on disjoint timesteps
    big = lambda lo: dict(timesteps=np.arange(lo, lo + 600), alphas=np.full(600, 0.5), alphas_prev=np.full(600, 0.6), sqrt_one_minus_alphas=np.full(600, 0.7))
    tab, distinct = step_table([big(0), big(300)])
    assert len(distinct) == 900 and tab.shape == (600, 2)
    with pytest.raises(MkdError, match='distinct timesteps'):
        step_table([big(0), big(600)])
    with pytest.raises(ValueError, match='solver'):
        step_table(good, 'euler')
    with pytest.raises(ValueError, match='entries for'):
        pack_sample_rows([dict(r(), alphas=[0.5, 0.5])])
    with pytest.raises(ValueError):
        pack_sample_rows([])


# ---- the draw-order rule -----------------------------------------------------------------------------------------------------------
def test_draw_order():
    m = StandIn()
    rows = build_rows([SampleSpec(10), SampleSpec(8, eta=0.5), SampleSpec(4, eta=1.0)], m.alphas_cumprod)
    plan = draw_plan(rows)
    # entry 0 of a DDIM grid has sigma > 0 too (alphas_prev[0] = alphas_cumprod[0]): steps 0 .. 7 draw, the 10-step sample alone draws nothing
    assert plan == [True] * 8 + [False] * 2
    assert draw_plan(rows[:1]) == [False] * 10 and draw_noise(rows[:1], (1, 4, 2, 2)) is None
    torch.manual_seed(5)
    nz = draw_noise(rows, (3, 4, 2, 2))
    torch.manual_seed(5)
    want = [torch.randn(3, 4, 2, 2) for _ in range(8)]
    after = torch.randn(2)
    assert tuple(nz.shape) == (10, 3, 4, 2, 2) and all(torch.equal(nz[k], want[k]) for k in range(8)) and not nz[8:].any()
    torch.manual_seed(5)
    draw_noise(rows, (3, 4, 2, 2))
    assert torch.equal(torch.randn(2), after)          # one draw per drawing step, nothing else consumed
    # a sigma that is zero in SOME steps: a hand-made row whose only non-zero sigma is in its entry 2 (executed step 1 of 4)
    hand = RowTables(np.array([1, 2, 3, 4]), *(np.full(4, v, dtype=np.float32) for v in (0.5, 0.6, 0.7)), sigmas=np.array([0, 0, 0.1, 0], dtype=np.float32))
    assert draw_plan([hand, rows[0]]) == [False, True] + [False] * 8
    # a finished sample's sigma does not count: entry 0 of the short row is non-zero, but it is only applied in ITS last step
    short = RowTables(np.array([1, 2]), *(np.full(2, v, dtype=np.float32) for v in (0.5, 0.6, 0.7)), sigmas=np.array([0.1, 0], dtype=np.float32))
    assert draw_plan([short, rows[0]]) == [False, True] + [False] * 8


def test_sampler_draws_x_T_then_the_steps():
    seen = {}

    class Model(StandIn):
        def sample_rows_fast(self, x, cond, rows, solver, uc, noise, temperature):
            seen.update(x=x, noise=noise, rows=rows, solver=solver, uc=uc, temperature=temperature)
            return x
    smp = DDIMSampler(Model())
    specs = [SampleSpec(4), SampleSpec(2, eta=1.0)]
    torch.manual_seed(11)
    smp.sample_specs(specs, (4, 2, 2), 'cond', temperature=0.5)
    torch.manual_seed(11)
    x = torch.randn(2, 4, 2, 2); d = [torch.randn(2, 4, 2, 2) for _ in range(2)]
    assert torch.equal(seen['x'], x) and torch.equal(seen['noise'][0], d[0]) and torch.equal(seen['noise'][1], d[1]) and not seen['noise'][2:].any()
    assert seen['solver'] == 'ddim' and seen['uc'] is None and seen['temperature'] == 0.5 and [r.n for r in seen['rows']] == [4, 2]
    DPMSolverSampler(Model()).sample_specs([SampleSpec(4, order=3), SampleSpec(5)], (4, 2, 2), 'cond', x_T=x)
    assert seen['solver'] == 'dpmpp' and seen['noise'] is None and seen['rows'][0].dpm.shape == (4, 6)


# ---- argument errors of the Python layer ---------------------------------------------------------------------------------------------
def test_python_argument_errors():
    for bad in (dict(steps=0), dict(steps=1025), dict(steps=2.5), dict(eta=-0.1), dict(eta=float('nan')), dict(guidance=float('inf')),
                dict(steps=10, t_start=0), dict(steps=10, t_start=11), dict(order=4)):
        with pytest.raises(ValueError):
            SampleSpec(**bad)
    m = StandIn()
    with pytest.raises(ValueError):
        build_rows([], m.alphas_cumprod)
    with pytest.raises(TypeError):
        build_rows([10], m.alphas_cumprod)
    with pytest.raises(ValueError, match='solver'):
        build_rows([SampleSpec()], m.alphas_cumprod, solver='plms')

    class Model(StandIn):
        def sample_rows_fast(self, *a):
            return a[0]
    smp = DDIMSampler(Model())
    with pytest.raises(ValueError, match='per sample'):
        smp.sample_specs([SampleSpec(4)], (4, 2, 2), None, unconditional_guidance_scale=9.0)
    with pytest.raises(ValueError, match='unconditional_conditioning'):
        smp.sample_specs([SampleSpec(4, guidance=2.0)], (4, 2, 2), None)
    with pytest.raises(ValueError, match='x_T'):
        smp.sample_specs([SampleSpec(4)], (4, 2, 2), None, x_T=torch.zeros(2, 4, 2, 2))
    with pytest.raises(NotImplementedError):
        DDIMSampler(StandIn()).sample_specs([SampleSpec(4)], (4, 2, 2), None)
    smp.make_schedule(10, verbose=False)
    x = torch.zeros(3, 4, 2, 2)
    with pytest.raises(ValueError, match='entries for a batch'):
        smp.decode(x, None, [3, 4])
    with pytest.raises(ValueError):
        smp.decode(x, None, [3, 4, 11])
    with pytest.raises(NotImplementedError):
        smp.decode(x, None, [3, 4, 5], callback=lambda i: None)
    smp.make_schedule(10, ddim_eta=0.5, verbose=False)
    with pytest.raises(NotImplementedError, match='deterministic'):
        smp.decode(x, None, torch.tensor([3, 4, 5]))
    assert smp.decode(x, None, 0) is x          # a scalar takes the old path


# ---- the float64 restatement of both updates against a loop of the single-request restatements ---------------------------------------
def _entries(rows, solver, k):
    return step_table(rows, solver)[0][k]


def test_ddim_rows_restatement_equals_a_loop_of_denoising_steps():
    m = StandIn()
    specs = [SampleSpec(10, guidance=9.0), SampleSpec(8, eta=0.5, guidance=1.0), SampleSpec(2, eta=1.0, guidance=3.0)]
    rows = build_rows(specs, m.alphas_cumprod)
    g = torch.Generator().manual_seed(3)
    x, e_c, e_u, nz = (torch.randn(3, 37, generator=g) for _ in range(4))
    for k in (0, 1, 2, 6, 9):
        en = _entries(rows, 'ddim', k)
        xp, p0, mag, mag0, active = pref.ddim_rows_fp64(x, e_c, e_u, en, nz, 0.7)
        assert active == [k < sp.steps for sp in specs]
        for b, sp in enumerate(specs):
            if not active[b]:
                assert torch.isnan(xp[b]).all() and torch.isnan(p0[b]).all()
                continue
            sch = sampler.Schedule().make_ddim(sp.steps, sp.eta)
            for name in ('ddim_alphas', 'ddim_alphas_prev', 'ddim_sigmas', 'ddim_sqrt_one_minus_alphas'):
                setattr(sch, name, getattr(sch, name).double())
            i = sp.steps - 1 - k
            e = e_u[b].double() + float(np.float32(sp.guidance)) * (e_c[b].double() - e_u[b].double())
            ref, ref0 = sampler.denoising_step(lambda *_: e.view(1, 1, 1, -1), sch, x[b].double().view(1, 1, 1, -1), None, None, i,
                                               temperature=float(np.float32(0.7)), noise=nz[b].double().view(1, 1, 1, -1))
            # the entry holds fp32 coefficients (four roundings of 2^-24 each, against the oracle's double square roots)
            assert torch.allclose(xp[b], ref.view(-1), rtol=0, atol=6 * 2 ** -24 * float(mag[b].max()))
            assert torch.allclose(p0[b], ref0.view(-1), rtol=0, atol=6 * 2 ** -24 * float(mag0[b].max()))
            assert (mag[b] >= xp[b].abs() * (1 - 1e-12)).all()


def test_dpm_rows_restatement_equals_a_loop_of_step_fp64():
    m = StandIn()
    specs = [SampleSpec(10, order=2, guidance=9.0), SampleSpec(5, order=3), SampleSpec(8, order=1, guidance=1.5)]
    rows = build_rows(specs, m.alphas_cumprod, solver='dpmpp')
    g = torch.Generator().manual_seed(4)
    x, e_c, e_u, m1, m2 = (torch.randn(3, 41, generator=g) for _ in range(5))
    for k in (0, 1, 2, 4, 5, 9):
        en = _entries(rows, 'dpmpp', k)
        xp, m0, mag, mag0, active = pref.dpm_rows_fp64(x, e_c, e_u, en, m1, m2)
        for b, sp in enumerate(specs):
            if k >= sp.steps:
                assert not active[b] and torch.isnan(xp[b]).all()
                continue
            ref, ref0, rmag, rmag0 = dref.step_fp64(x[b], e_c[b], e_u[b], sp.guidance, rows[b].dpm[sp.steps - 1 - k], m1[b], m2[b])
            assert torch.equal(xp[b], ref) and torch.equal(m0[b], ref0) and torch.equal(mag[b], rmag) and torch.equal(mag0[b], rmag0)
    # without an unconditional half the scale is not used
    xp, *_ = pref.dpm_rows_fp64(x, e_c, None, _entries(rows, 'dpmpp', 0), m1, m2)
    ref, *_ = dref.step_fp64(x[1], e_c[1], None, 1.0, rows[1].dpm[4], m1[1], m2[1])
    assert torch.equal(xp[1], ref)


def test_restated_loops_reduce_to_the_uniform_loops():
    """the restated per-sample loops with a stand-in eps that treats rows independently: row b is the single-request loop's row"""
    eps_fn = lambda x, t, c: torch.tanh(x * 0.5 + t.view(-1, 1, 1, 1).float() / 1000.0) * (1.0 if c is None else c)
    g = torch.Generator().manual_seed(9)
    x_T = torch.randn(3, 4, 2, 2, generator=g)
    steps = (10, 7, 4)
    schs = [sampler.Schedule().make_ddim(s, eta) for s, eta in zip(steps, (0.5, 0.0, 1.0))]
    nz = torch.randn(10, 3, 4, 2, 2, generator=g)
    out = pref.ddim_loop_rows(eps_fn, schs, steps, x_T, None, noise=nz, temperature=0.9)
    for b in range(3):
        img = x_T[b:b + 1]
        for k in range(steps[b]):
            i = steps[b] - 1 - k
            ts = torch.full((1,), int(schs[b].ddim_timesteps[i]), dtype=torch.long)
            img, _ = sampler.denoising_step(eps_fn, schs[b], img, None, ts, i, temperature=0.9, noise=nz[k, b:b + 1])
        assert torch.equal(out[b:b + 1], img), b
    grids = [dref.grid(s) for s in (10, 5, 8)]
    out = pref.dpm_loop_rows(eps_fn, grids, (2, 3, 1), x_T, None)
    for b, o in enumerate((2, 3, 1)):
        ref = dref.dpm_solver_pp(eps_fn, *grids[b], x_T[b:b + 1], None, order=o)
        assert torch.equal(out[b:b + 1], ref), b
