"""-m gpu: per-sample requests in one batch (mkd_sample_rows).  The two row kernels alone against float64, the row independence of
the existing loop (the precondition of everything below), the bit contract against the uniform entries in every loop form, the
per-sample start point of decode / reconstruct, the host-driven loop, the launch count, the refusals, the trajectories against the
oracle nets, and the model surface (transfer_specs, runs/test.py --steps-list)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dpm_solver_ref as dref
import per_sample_ref as pref
import vae_encoder_ref as enc_ref
from gpu_util import DEV, sync
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd.batching import SampleSpec, build_rows
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.diffmk.cddim import MKDDIMSampler
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler
from makeupdiffuse_amd.engine import MkdEngine, NetConfig, step_table
from makeupdiffuse_amd.lib import MkdError
from oracle import nets, sampler, vae

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the small nets of test_gpu_sample_extras.py
NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))
B = 3
AC = sampler.Schedule().alphas_cumprod          # the fp32 DDPM table every sampler here indexes

# Limits of the per-sample trajectories (DESIGN.md section 2 convention: per sample, rel-L2 at most 3 x the distance measured on the
# MI355X for that case and sample, cosine >= 0.99): small nets, B = 3, 8x8 latents, the device loop against the restated per-sample
# loop over the fp32 oracle nets.  One number per sample of the case, in batch order
MEASURED = {
    'ddim plain (10, 7, 4)': (3.6090e-3, 4.3145e-3, 5.2916e-3),
    'ddim guided (10 s9, 4 s9, 10 s1.5)': (2.4861e-2, 2.6101e-2, 5.1883e-3),
    'dpm2 plain (10, 7, 4)': (3.4885e-3, 3.8613e-3, 4.3750e-3),
}
COS_CAP = 0.99


def metrics(out, ref):
    out = out.float().cpu(); ref = ref.float().cpu()
    assert torch.isfinite(out).all(), 'non-finite output'
    return ((out - ref).norm() / ref.norm()).item(), F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()


def small_engine(sd):
    eng = MkdEngine(NetConfig(hint_channels=6, model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2,
                              context_dim=64, hint_widths=tuple(HINT_WIDTHS)))
    eng.load_state_dict(sd)
    return eng


@pytest.fixture(scope='module')
def sd():
    return nets.init_state_dict(OCFG, seed=31)


@pytest.fixture(scope='module')
def engines(sd):
    """(a context with the default single-graph replay, one whose replay runs as per-stream linear segments)"""
    one = small_engine(sd)
    old = os.environ.get('MKD_GRAPH_MODE')
    os.environ['MKD_GRAPH_MODE'] = '2'
    try:
        seg = small_engine(sd)
    finally:
        if old is None:
            del os.environ['MKD_GRAPH_MODE']
        else:
            os.environ['MKD_GRAPH_MODE'] = old
    yield one, seg
    one.close(); seg.close()


@pytest.fixture(scope='module')
def mm(sd):
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True,
                         ddim_steps=8, unconditional_guidance_scale=9)
    m.load_state_dict({**sd, **vae.init_state_dict(vcfg, seed=32), **enc_ref.init_state_dict(vcfg, seed=33)})
    m.cuda(0)
    g = torch.Generator().manual_seed(34)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=g)
    m.save_images = False
    return m


def inputs(seed=35, res=64):
    g = torch.Generator().manual_seed(seed)
    h = res // 8
    return dict(hint=torch.rand(B, 6, res, res, generator=g).to(DEV), ctx=torch.randn(B, 77, 64, generator=g).to(DEV),
                uctx=torch.randn(B, 77, 64, generator=g).to(DEV), x_T=torch.randn(B, 4, h, h, generator=g).to(DEV))


def prepare(eng, I, guided):
    if guided:
        eng.prepare(torch.cat([I['hint'], I['hint']]), torch.cat([I['uctx'], I['ctx']]))
    else:
        eng.prepare(I['hint'], I['ctx'])


def uniform(eng, x_T, row, solver, order, use_graph, noise=None):
    """today's uniform entry with one sample's request"""
    if solver == 'dpmpp':
        return eng.sample_dpmpp(x_T, row.timesteps, row.alphas, row.alphas_prev, order=order, cfg_scale=row.cfg_scale, use_graph=use_graph)
    kw = {} if row.sigmas is None else dict(sigmas=row.sigmas, noise=noise[:row.n])
    return eng.sample(x_T, row.timesteps, row.alphas, row.alphas_prev, row.sqrt_one_minus_alphas, cfg_scale=row.cfg_scale,
                      use_graph=use_graph, **kw)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the row kernels alone -----------------------------------------------------------------------------------------------------
PATTERN = 0x7FC12345          # a NaN with a payload: any write to a finished row shows


def patterned(n):
    return torch.full((n,), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)


def kernel_rows(solver):
    """entries of an executed step in which sample 0 is guided, sample 1 runs with s = 1 (and an eps_u) and sample 2 has finished"""
    if solver == 'ddim':
        specs = [SampleSpec(10, eta=0.5, guidance=9.0), SampleSpec(10, eta=1.0, guidance=1.0), SampleSpec(4)]
    else:
        specs = [SampleSpec(10, order=2, guidance=9.0), SampleSpec(10, order=3, guidance=1.0), SampleSpec(4, order=1)]
    tab, _ = step_table(build_rows(specs, AC, solver), solver)
    return tab


@pytest.mark.parametrize('per', [256, 100, 105])          # 4 * 8 * 8; 4 * 5 * 5 (16-byte form, not a multiple of the block); the scalar form
def test_ddim_row_kernel_against_fp64(engines, per):
    """|err| <= 8 * 2^-24 * the magnitude sum per element, test_gpu_dpm_solver.py's bound for the uniform kernels (at most eight fp32
    roundings: two of the guidance combine, two of x0, two of the sum, two of the noise term), x_prev against c1 |p0| + c2 |e| +
    |sigma z T| and pred_x0 against (|x| + c3 (|e_u| + |s (e_c - e_u)|)) c0.  The finished row's eps is NaN; its x_prev / pred_x0
    rows come back with their bit pattern."""
    eng, _ = engines
    tab = kernel_rows('ddim')
    g = torch.Generator().manual_seed(per)
    for k in (5, 9):
        en = tab[k]
        assert list(en['active']) == [1, 1, 0] and en['scale'][1] == 1.0 and (en['sigma'][:2] != 0).all()
        x, e_c, e_u, nz = (torch.randn(B, per, generator=g) for _ in range(4))
        e_c[2] = float('nan'); e_u[2] = float('nan')
        xp = patterned(B * per).view(B, per); p0 = patterned(B * per).view(B, per)
        eng.ddim_step_rows(x.to(DEV), e_c.to(DEV), e_u.to(DEV), en, noise=nz.to(DEV), temperature=0.8, x_prev=xp, pred_x0=p0)
        sync()
        ref, ref0, mag, mag0, active = pref.ddim_rows_fp64(x, e_c, e_u, en, nz, 0.8)
        for b in (0, 1):
            err, err0 = (xp[b].cpu().double() - ref[b]).abs(), (p0[b].cpu().double() - ref0[b]).abs()
            print(f'[ddim rows] per {per} step {k} sample {b}: x {(err / mag[b]).max().item() / 2 ** -24:.2f}, x0 {(err0 / mag0[b]).max().item() / 2 ** -24:.2f} x 2^-24')
            assert (err <= 8 * 2 ** -24 * mag[b]).all() and (err0 <= 8 * 2 ** -24 * mag0[b]).all()
        assert (bits(xp[2]) == PATTERN).all() and (bits(p0[2]) == PATTERN).all(), 'a finished row was written'
        # without an unconditional half, without noise, without pred_x0, in place: the same kernel's other branches
        xi = x.to(DEV).clone()
        eng.ddim_step_rows(xi, e_c.to(DEV), None, en, x_prev=xi, want_x0=False)
        sync()
        r2, _, m2, _, _ = pref.ddim_rows_fp64(x, e_c, None, en)
        assert ((xi[:2].cpu().double() - r2[:2]).abs() <= 8 * 2 ** -24 * m2[:2]).all() and torch.equal(xi[2].cpu(), x[2])


@pytest.mark.parametrize('per', [256, 100, 105])
def test_dpm_row_kernel_against_fp64(engines, per):
    """the same bound for the DPM-Solver++ rows (dpmpp_update_at's arithmetic) on the rows the bound is stated for: a guided sample
    (order 2), one with s = 1 and an eps_u (order 3), one that has finished; the finished sample's x, ring (m0) and output rows keep
    their bit pattern although its eps is NaN.  (The magnitude sum takes |c_0 m0| with the computed m0, as the uniform kernels' test
    does: where x - sigma e cancels AND c_x is small - the last entries of a 4-step grid at order 1 - the rounding of m0 alone can
    exceed it, for the uniform kernel as for this one; those entries are covered by the bit contract instead.)"""
    eng, _ = engines
    tab = kernel_rows('dpmpp')
    g = torch.Generator().manual_seed(per + 1)
    for k in (4, 6, 9):
        en = tab[k]
        assert list(en['active']) == [1, 1, 0]
        x, e_c, e_u, m1, m2 = (torch.randn(B, per, generator=g) for _ in range(5))
        fin = not en['active'][2]
        if fin:
            e_c[2] = float('nan'); e_u[2] = float('nan')
        xp = patterned(B * per).view(B, per); m0 = patterned(B * per).view(B, per)
        eng.dpmpp_step_rows(x.to(DEV), e_c.to(DEV), e_u.to(DEV), en, m1.to(DEV), m2.to(DEV), x_prev=xp, m0=m0)
        sync()
        ref, ref0, mag, mag0, _ = pref.dpm_rows_fp64(x, e_c, e_u, en, m1, m2)
        for b in range(B):
            if not en['active'][b]:
                continue
            err, err0 = (xp[b].cpu().double() - ref[b]).abs(), (m0[b].cpu().double() - ref0[b]).abs()
            print(f'[dpm rows] per {per} step {k} sample {b}: x {(err / mag[b]).max().item() / 2 ** -24:.2f}, m0 {(err0 / mag0[b]).max().item() / 2 ** -24:.2f} x 2^-24')
            assert (err <= 8 * 2 ** -24 * mag[b]).all() and (err0 <= 8 * 2 ** -24 * mag0[b]).all()
        if fin:
            assert (bits(xp[2]) == PATTERN).all() and (bits(m0[2]) == PATTERN).all(), 'a finished row was written'
            # in place, the loop's form: x and the ring slot of a finished sample are left as they are
            xi = x.to(DEV).clone(); xi[2] = patterned(per); ring = patterned(B * per).view(B, per)
            eng.dpmpp_step_rows(xi, e_c.to(DEV), e_u.to(DEV), en, m1.to(DEV), m2.to(DEV), x_prev=xi, m0=ring)
            sync()
            assert torch.equal(xi[:2], xp[:2]) and (bits(xi[2]) == PATTERN).all() and (bits(ring[2]) == PATTERN).all()


@pytest.mark.parametrize('per', [256, 100])
def test_row_kernels_scalar_and_vector_forms_give_the_same_bits(engines, per):
    """pointers 4 bytes off take the scalar form: the same bits as the 16-byte form on the same elements"""
    eng, _ = engines
    g = torch.Generator().manual_seed(17)
    bufs = [torch.randn(B * per + 1, generator=g).to(DEV) for _ in range(6)]
    for solver in ('ddim', 'dpmpp'):
        en = kernel_rows(solver)[2]          # every sample active
        res = []
        for aligned in (True, False):
            ts = [(b[1:].clone() if aligned else b[1:]).view(B, per) for b in bufs]
            assert all((t.data_ptr() % 16 == 0) == aligned for t in ts)
            o1, o2 = (torch.zeros(B * per + 1, device=DEV)[1:].view(B, per) for _ in range(2))
            if aligned:
                o1, o2 = o1.clone(), o2.clone()
            assert (o1.data_ptr() % 16 == 0) == aligned
            x, e_c, e_u, a, b_, _ = ts
            if solver == 'ddim':
                eng.ddim_step_rows(x, e_c, e_u, en, noise=a, temperature=0.9, x_prev=o1, pred_x0=o2)
            else:
                eng.dpmpp_step_rows(x, e_c, e_u, en, a, b_, x_prev=o1, m0=o2)
            sync()
            res.append((o1.clone(), o2.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), solver
        assert torch.isfinite(res[0][0]).all() and res[0][0].abs().sum() > 0


# ---- 2. row independence of the existing loop (the precondition; passes before this feature) ------------------------------------------
@pytest.mark.parametrize('guided', [False, True])
def test_uniform_loop_rows_are_independent(engines, guided):
    """a uniform 10-step call, then the same call with rows 1 and 2 of x_T, hint and context replaced: row 0 keeps its bits"""
    one, _ = engines
    I, J = inputs(35), inputs(36)
    row = build_rows([SampleSpec(10, guidance=9.0 if guided else 1.0)], AC)[0]
    prepare(one, I, guided)
    a = uniform(one, I['x_T'], row, 'ddim', 2, True)
    M = {k: torch.cat([I[k][:1], J[k][1:]]) for k in I}
    prepare(one, M, guided)
    b = uniform(one, M['x_T'], row, 'ddim', 2, True)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])


# ---- 3. the bit contract ------------------------------------------------------------------------------------------------------------------
CASES = {
    'plain': ('ddim', [SampleSpec(10), SampleSpec(7), SampleSpec(4)]),
    'guidance': ('ddim', [SampleSpec(10, guidance=9.0), SampleSpec(7, guidance=1.5), SampleSpec(4, guidance=3.0)]),
    'eta': ('ddim', [SampleSpec(10, eta=0.5), SampleSpec(7), SampleSpec(4, eta=1.0)]),
    'dpm': ('dpmpp', [SampleSpec(10, order=2), SampleSpec(5, order=3), SampleSpec(8, order=1)]),
}


def case_noise(specs):
    g = torch.Generator().manual_seed(77)
    return torch.randn(max(s.steps for s in specs), B, 4, 8, 8, generator=g).to(DEV)


@pytest.mark.parametrize('form', ['graph', 'segments', 'eager'])
@pytest.mark.parametrize('case', list(CASES))
def test_bit_contract(engines, case, form):
    """row b of the per-sample call has the bits of row b of the uniform call with sample b's request (schedule, scale, rows
    0 .. n_b - 1 of the noise), on the same context, prepared batch and loop form"""
    one, seg = engines
    eng, use_graph = (seg, True) if form == 'segments' else (one, form == 'graph')
    solver, specs = CASES[case]
    I = inputs()
    rows = build_rows(specs, AC, solver)
    guided = any(s.guidance != 1.0 for s in specs)
    noise = case_noise(specs) if case == 'eta' else None
    prepare(eng, I, guided)
    out = eng.sample_rows(I['x_T'], rows, solver=solver, noise=noise, use_graph=use_graph)
    assert torch.isfinite(out).all()
    refs = [uniform(eng, I['x_T'], rows[b], solver, specs[b].order, use_graph, noise) for b in range(B)]
    for b in range(B):
        assert torch.equal(out[b], refs[b][b]), f'{case} / {form}: row {b} ({specs[b]})'
        other = refs[(b + 1) % B][b]
        assert metrics(out[b], other)[0] > 1e-2, f'{case}: row {b} does not depend on its request'
    # ... and again (the captured step is replayed, the table is rewritten), also after every scratch buffer was poisoned
    assert torch.equal(eng.sample_rows(I['x_T'], rows, solver=solver, noise=noise, use_graph=use_graph), out)
    eng.debug_poison()
    assert torch.equal(eng.sample_rows(I['x_T'], rows, solver=solver, noise=noise, use_graph=use_graph), out), 'poisoned'


@pytest.mark.parametrize('form', ['graph', 'segments', 'eager'])
def test_uniform_and_per_sample_calls_alternate(sd, engines, form, monkeypatch):
    """a uniform call after a per-sample call (and the reverse) gives the bits it gives on a fresh context"""
    one, seg = engines
    eng, use_graph = (seg, True) if form == 'segments' else (one, form == 'graph')
    I = inputs()
    if form == 'segments':
        monkeypatch.setenv('MKD_GRAPH_MODE', '2')
    fresh = small_engine(sd)
    try:
        for solver, specs in (CASES['guidance'], CASES['dpm']):
            guided = any(s.guidance != 1.0 for s in specs)
            rows = build_rows(specs, AC, solver)
            prepare(fresh, I, guided)
            want_u = uniform(fresh, I['x_T'], rows[0], solver, specs[0].order, use_graph)
            fresh.debug_poison()
            want_r = fresh.sample_rows(I['x_T'], rows, solver=solver, use_graph=use_graph)          # the first loop of its kind on that context
            prepare(eng, I, guided)
            for _ in range(2):
                assert torch.equal(eng.sample_rows(I['x_T'], rows, solver=solver, use_graph=use_graph), want_r), solver
                assert torch.equal(uniform(eng, I['x_T'], rows[0], solver, specs[0].order, use_graph), want_u), solver
    finally:
        fresh.close()


# ---- 4. per-sample start point ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 9.0])
def test_decode_with_a_start_point_per_sample(mm, scale):
    """decode / reconstruct with t_start = (6, 3, 10) of a 10-step schedule: row b is row b of the scalar call with t_start_b"""
    I = inputs()
    c = {'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]}
    uc = {'c_crossattn': [I['uctx']], 'c_concat': [I['hint']]} if scale != 1.0 else None
    starts = (6, 3, 10)
    for cls, method in ((DDIMSampler, 'decode'), (MKDDIMSampler, 'reconstruct')):
        smp = cls(mm)
        smp.make_schedule(10, verbose=False)
        run = lambda t: getattr(smp, method)(I['x_T'], c, t, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
        outs = [run(starts), run(torch.tensor(starts)), run(np.asarray(starts))]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        refs = [run(t) for t in starts]
        for b in range(B):
            assert torch.equal(outs[0][b], refs[b][b]), f'{method} scale {scale}: row {b}'
        assert metrics(outs[0][1], refs[0][1])[0] > 1e-2


# ---- 5. the host-driven loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', ['ddim', 'dpmpp'])
def test_host_driven_loop_equals_the_in_library_loop(engines, solver):
    """per step eng.eps with the samples' own timesteps, then the stand-alone row kernel: the in-library loop's bits.  Sample 1 runs
    with s = 1 inside a guided batch (the uniform entries cannot: cfg_scale = 1 there means a batch-B plan)"""
    one, _ = engines
    I = inputs()
    if solver == 'ddim':
        specs = [SampleSpec(10, eta=0.5, guidance=9.0), SampleSpec(7, guidance=1.0), SampleSpec(4, eta=1.0, guidance=3.0)]
    else:
        specs = [SampleSpec(10, order=2, guidance=9.0), SampleSpec(5, order=3, guidance=1.0), SampleSpec(8, order=1, guidance=3.0)]
    rows = build_rows(specs, AC, solver)
    noise = case_noise(specs) if solver == 'ddim' else None
    prepare(one, I, True)
    outs = [one.sample_rows(I['x_T'], rows, solver=solver, noise=noise, use_graph=g) for g in (True, False)]
    assert torch.equal(outs[0], outs[1])
    tab, _ = step_table(rows, solver)
    x = I['x_T'].clone()
    ring = [patterned(x.numel()).view_as(x).clone() for _ in range(3)]
    for k in range(tab.shape[0]):
        t = torch.from_numpy(tab[k]['t'].astype(np.int64))
        e_u, e_c = one.eps(torch.cat([x, x]), torch.cat([t, t])).chunk(2)
        if solver == 'ddim':
            one.ddim_step_rows(x, e_c, e_u, tab[k], noise=noise[k], x_prev=x, want_x0=False)
        else:
            one.dpmpp_step_rows(x, e_c, e_u, tab[k], ring[(k + 2) % 3], ring[(k + 1) % 3], x_prev=x, m0=ring[k % 3])
    assert torch.equal(x, outs[0])
    assert metrics(x[1], I['x_T'][1])[0] > 1e-2


# ---- 6. launch count ----------------------------------------------------------------------------------------------------------------------
def test_step_launch_count(engines):
    """a per-sample step is setup, evaluation and update (+ the batch doubling): the replayed uniform step's count for the same guidance
    form, captured or not; the uniform counts do not move"""
    one, _ = engines
    I = inputs()
    prepare(one, I, True)
    before = [one.step_launches(g, c) for g in (True, False) for c in (False, True)]
    for cfg in (False, True):
        for g in (True, False):
            assert one.step_launches(g, cfg, per_sample=True) == one.step_launches(True, cfg)
        assert one.lib.mkd_step_launches_ex(one._ctx, 1, mlib.STEP_PER_SAMPLE | int(cfg)) == one.lib.mkd_step_launches_ex(one._ctx, 1, int(cfg))
    assert one.step_launches(True, True, per_sample=True) == one.step_launches(True, False, per_sample=True) + 1
    solver, specs = CASES['guidance']
    one.sample_rows(I['x_T'], build_rows(specs, AC, solver), use_graph=True)
    assert [one.step_launches(g, c) for g in (True, False) for c in (False, True)] == before
    with pytest.raises(ValueError):
        one.step_launches(True, True, rescale=True, per_sample=True)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(engines):
    one, _ = engines
    I = inputs()
    rows = build_rows(CASES['plain'][1], AC)
    prepare(one, I, False)
    want = uniform(one, I['x_T'], rows[0], 'ddim', 2, True)
    d = lambda row, **kw: dict(timesteps=row.timesteps, alphas=row.alphas, alphas_prev=row.alphas_prev,
                               sqrt_one_minus_alphas=row.sqrt_one_minus_alphas, cfg_scale=row.cfg_scale, **kw)
    big = lambda lo: dict(timesteps=np.arange(lo, lo + 600), alphas=np.full(600, 0.5), alphas_prev=np.full(600, 0.6), sqrt_one_minus_alphas=np.full(600, 0.7))
    guided_rows = build_rows(CASES['guidance'][1], AC)
    dpm_rows = build_rows(CASES['dpm'][1], AC, 'dpmpp')
    ARG, UNSUPPORTED = r'\(-1\)', r'\(-4\)'
    cases = [
        (dict(rows=[d(rows[0], n_steps=0), rows[1], rows[2]]), ARG, 'sample 0: n_steps must be >= 1'),
        (dict(rows=[rows[0], d(rows[1], n_steps=1025), rows[2]]), ARG, 'sample 1: n_steps exceeds MKD_MAX_STEPS'),
        (dict(rows=[rows[0], rows[1], dict(d(rows[2]), alphas_prev=None)]), ARG, 'sample 2: null table'),
        (dict(rows=[d(r) for r in dpm_rows], solver='dpmpp'), ARG, 'sample 0: null table'),          # DDIM tables alone, no mkd_dpmpp_table rows
        (dict(rows=[rows[0], d(rows[1], sigmas=[0.0] * (rows[1].n - 1) + [1.5]), rows[2]], noise=torch.zeros(10, B, 4, 8, 8)), ARG, 'sample 1: sigma out of range'),
        (dict(rows=guided_rows), ARG, 'prepared batch must be B'),
        (dict(rows=[big(0), big(600), rows[2]]), ARG, 'more than MKD_MAX_STEPS distinct timesteps'),
        (dict(rows=rows, x0=I['x_T'], mask=torch.ones(1, 1, 8, 8, device=DEV)), UNSUPPORTED, 'combined with masked sampling'),
        (dict(rows=rows, want_trace=True), UNSUPPORTED, 'combined with the intermediates trace'),
        (dict(rows=rows, guidance_rescale=0.7), UNSUPPORTED, 'combined with guidance rescale'),
    ]
    for use_graph in (True, False):
        for kw, code, msg in cases:
            with pytest.raises(MkdError, match=code + '.*' + msg):
                one.sample_rows(I['x_T'], use_graph=use_graph, **kw)
            assert msg in one.lib.mkd_last_error().decode()
        assert torch.equal(uniform(one, I['x_T'], rows[0], 'ddim', 2, use_graph), uniform(one, I['x_T'], rows[0], 'ddim', 2, use_graph))
    assert torch.equal(uniform(one, I['x_T'], rows[0], 'ddim', 2, True), want)
    # the Python layer: the latent must match the rows and the prepared size, eta > 0 needs its draws
    with pytest.raises(ValueError, match='x_T'):
        one.sample_rows(I['x_T'][:2], rows)
    with pytest.raises(ValueError, match='noise'):
        one.sample_rows(I['x_T'], build_rows(CASES['eta'][1], AC))
    with pytest.raises(ValueError, match='noise'):
        one.sample_rows(I['x_T'], build_rows(CASES['eta'][1], AC), noise=torch.zeros(9, B, 4, 8, 8))
    with pytest.raises(ValueError, match='solver'):
        one.sample_rows(I['x_T'], rows, solver='plms')
    # the stand-alone kernels' checks
    en = kernel_rows('ddim')[0]
    z = torch.zeros(B, 16, device=DEV)
    with pytest.raises(ValueError):
        one.ddim_step_rows(z, z, None, en[:2])
    with pytest.raises(ValueError):
        one.ddim_step_rows(z, z[:, :8].contiguous(), None, en)
    assert one.lib.mkd_ddim_step_rows(z.data_ptr(), z.data_ptr(), None, None, None, 1.0, z.data_ptr(), None, B, 16, None) == -1
    assert one.lib.mkd_dpmpp_step_rows(z.data_ptr(), z.data_ptr(), None, z.data_ptr(), None, None, z.data_ptr(), z.data_ptr(), B, 16, None) == -1
    assert one.lib.mkd_ddim_step_rows(z.data_ptr(), z.data_ptr(), None, z.data_ptr(), None, 1.0, z.data_ptr(), None, 0, 16, None) == -1


# ---- 8. against the oracle ------------------------------------------------------------------------------------------------------------------
def oracle_case(name, sd_, I):
    """(device run, restated run) of a case; both take a list of per-sample (steps, scale) and return the latent"""
    cpu = lambda d: {k: [t.cpu() for t in v] for k, v in d.items()}
    c = cpu({'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]})
    uc = cpu({'c_crossattn': [I['uctx']], 'c_concat': [I['hint']]})
    eps_fn = sampler.make_eps_fn(sd_, OCFG)
    x_T = I['x_T'].cpu()
    if name.startswith('ddim'):
        def restated(req):
            schs = [sampler.Schedule().make_ddim(s) for s, _ in req]
            return pref.ddim_loop_rows(eps_fn, schs, [len(s.ddim_timesteps) for s in schs], x_T, c, [g for _, g in req], uc)          # (S = 7: upstream's 8-entry grid, all of it)
    else:
        def restated(req):
            grids = []
            for s, _ in req:
                sch = sampler.Schedule().make_ddim(s)
                grids.append((sch.ddim_timesteps, sch.ddim_alphas.numpy(), sch.ddim_alphas_prev.numpy()))
            return pref.dpm_loop_rows(eps_fn, grids, [2] * len(req), x_T, c, [g for _, g in req], uc)
    return restated


ORACLE_CASES = {
    'ddim plain (10, 7, 4)': ('ddim', [(10, 1.0), (7, 1.0), (4, 1.0)]),
    'ddim guided (10 s9, 4 s9, 10 s1.5)': ('ddim', [(10, 9.0), (4, 9.0), (10, 1.5)]),
    'dpm2 plain (10, 7, 4)': ('dpmpp', [(10, 1.0), (7, 1.0), (4, 1.0)]),
}


@pytest.mark.parametrize('name', list(ORACLE_CASES))
def test_per_sample_trajectory_vs_oracle(engines, sd, name):
    """Per sample: rel-L2 <= 3 x the distance measured on the MI355X for that case and sample (MEASURED), cosine >= 0.99, against the
    restated per-sample loop over the fp32 oracle nets.  Asserted FIRST: every restated row lies >= 3 x its limit from the row the
    same sample gets under each OTHER request of its case, so a loop that ignores the per-sample rows cannot pass."""
    one, _ = engines
    solver, req = ORACLE_CASES[name]
    I = inputs()
    restated = oracle_case(name, sd, I)
    ref = restated(req)
    specs = [SampleSpec(s, guidance=g, order=2) for s, g in req]
    guided = any(g != 1.0 for _, g in req)
    prepare(one, I, guided)
    out = one.sample_rows(I['x_T'], build_rows(specs, AC, solver), solver=solver, use_graph=True).cpu()
    got = [metrics(out[b], ref[b]) for b in range(B)]
    # the rows the same samples get when EVERY sample runs one of the case's other requests
    others = {r: restated([r] * B) for r in dict.fromkeys(req)}
    apart = [min(metrics(ref[b], others[r][b])[0] for r in others if r != req[b]) for b in range(B)]
    print(f'[parity] per-sample {name}: rel-L2 ' + ', '.join(f'{r:.4e}' for r, _ in got) + '; cos ' + ', '.join(f'{c:.6f}' for _, c in got) +
          '; restated row vs its nearest other request ' + ', '.join(f'{a:.3f}' for a in apart))
    assert MEASURED[name] is not None, 'no measured distance recorded'
    for b in range(B):
        lim = 3.0 * MEASURED[name][b]
        assert apart[b] >= 3.0 * lim, f'precondition, sample {b}: restated row {apart[b]:.4f} from another request < 3 x limit {lim:.4f}'
    for b in range(B):
        r, cs = got[b]
        assert cs >= COS_CAP and r <= 3.0 * MEASURED[name][b], f'sample {b}: rel-L2 {r:.4e} > {3.0 * MEASURED[name][b]:.4e} or cos {cs:.6f}'


# ---- 9. the model surface -------------------------------------------------------------------------------------------------------------------
def test_transfer_specs(mm):
    m = mm
    g = torch.Generator().manual_seed(70)
    batch = {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g),
             'txt_emb': torch.randn(B, 77, 64, generator=g)}
    x_T = torch.randn(B, 4, 8, 8, generator=g).to(DEV)
    hint = torch.cat((batch['src_img'], batch['ref_img']), 1).to(DEV)
    ctx = batch['txt_emb'].to(DEV)

    def uniform_rows(idx, steps, scale, order=2):
        """the class path of today on the sub-batch idx: (S = steps, scale) for all of them"""
        sel = torch.as_tensor(idx, device=DEV)
        c = {'c_concat': [hint[sel].contiguous()], 'c_crossattn': [ctx[sel].contiguous()]}
        kw = {}
        if scale != 1.0:
            kw = dict(unconditional_guidance_scale=scale,
                      unconditional_conditioning={'c_concat': c['c_concat'], 'c_crossattn': [m.get_unconditional_conditioning(len(idx))]})
        if m.sampler == 'dpmpp':
            return DPMSolverSampler(m).sample(steps, len(idx), (4, 8, 8), c, x_T=x_T[sel].contiguous(), order=order, **kw)[0]
        return DDIMSampler(m).sample(steps, len(idx), (4, 8, 8), c, x_T=x_T[sel].contiguous(), verbose=False, **kw)[0]
    try:
        for smp_name in ('ddim', 'dpmpp'):
            m.sampler = smp_name
            # one form: every sample unguided
            specs = [SampleSpec(10), SampleSpec(7), SampleSpec(4)]
            out = m.transfer_specs(batch, specs, x_T=x_T)
            assert set(out) == {'samples_latent', 'samples'} and tuple(out['samples'].shape) == (B, 3, 64, 64)
            for b, sp in enumerate(specs):
                assert torch.equal(out['samples_latent'][b], uniform_rows([0, 1, 2], sp.steps, 1.0)[b]), (smp_name, b)
            assert torch.equal(out['samples'], m.decode_first_stage(out['samples_latent']))
            # two forms: samples 0 and 2 guided (one pass on [uncond; cond] of those two), sample 1 not (a pass of its own)
            specs = [SampleSpec(10, guidance=9.0), SampleSpec(7), SampleSpec(4, guidance=1.5)]
            out = m.transfer_specs(batch, specs, x_T=x_T)
            assert torch.equal(out['samples_latent'][0], uniform_rows([0, 2], 10, 9.0)[0]), smp_name
            assert torch.equal(out['samples_latent'][2], uniform_rows([0, 2], 4, 1.5)[1]), smp_name
            assert torch.equal(out['samples_latent'][1], uniform_rows([1], 7, 1.0)[0]), smp_name
            assert torch.isfinite(out['samples']).all()
    finally:
        m.sampler = 'ddim'
    with pytest.raises(ValueError, match='one SampleSpec per pair'):
        m.transfer_specs(batch, [SampleSpec(4)] * 2)
    # the sampler methods themselves, with eta > 0: the draws are x_T, then one per drawing step
    c = {'c_concat': [hint], 'c_crossattn': [ctx]}
    specs = [SampleSpec(10, eta=0.5), SampleSpec(4), SampleSpec(5, eta=1.0)]
    torch.manual_seed(3)
    a = DDIMSampler(m).sample_specs(specs, (4, 8, 8), c)
    torch.manual_seed(3)
    x = torch.randn(B, 4, 8, 8, device=DEV)
    nz = torch.stack([torch.randn(B, 4, 8, 8, device=DEV) for _ in range(10)])
    rows = build_rows(specs, m.alphas_cumprod)
    m.reset_conditioning_cache()
    eng = m._bind_cond(c, (8, 8))
    assert torch.equal(a, eng.sample_rows(x, rows, noise=nz, use_graph=True))


def test_runs_test_py_steps_list(tmp_path):
    from PIL import Image
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--pairs', '2', '--batch-size', '2', '--res', '64',
                        '--ddim-steps', '4', '--seed', '5', '--steps-list', '4,8', '--out', str(out)],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    root = out / 'makeupdiffuse_mi355x'
    names = sorted(os.listdir(root))
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'samples_0000.png', 'samples_cfg_scale_9.00_0000.png',
                     'samples_specs_0000.png'], names
    assert np.asarray(Image.open(root / 'samples_specs_0000.png')).std() > 1.0
    lat = torch.load(out / 'latents_0000.pt')
    assert tuple(lat['samples_specs_latent'].shape) == (2, 4, 8, 8) and tuple(lat['samples_specs'].shape) == (2, 3, 64, 64)
    # pair 0 ran the 4 steps of the plain pass from the same x_T: the same latent; pair 1 ran 8
    assert torch.equal(lat['samples_specs_latent'][0], lat['samples_latent'][0])
    assert not torch.equal(lat['samples_specs_latent'][1], lat['samples_latent'][1])
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--steps-list', '4,x'], capture_output=True, text=True,
                       timeout=900, cwd=str(tmp_path))
    assert r.returncode != 0 and '--steps-list' in r.stderr
