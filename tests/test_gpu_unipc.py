"""-m gpu: the UniPC predictor-corrector sampler on the device.  The step kernel against the float64 restatement per element, its
vector and scalar forms, every loop form (graph replay, linear graph segments, eager) against the per-step class loop bit for bit,
the corrector-free order 2 against the DPM-Solver++ loop of the same context, the order-2 trajectory against the oracle nets inside
the restated solver, the trace and the guidance rescale, the state DDIM, DPM-Solver++ and UniPC calls share on one context, the
step-launch count, the masked refusal, and the model surface (TestDiffuseModel(sampler='unipc'), runs/test.py --sampler unipc)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dpm_solver_ref as dref
import unipc_ref as uref
import vae_encoder_ref as enc_ref
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd.ddim import rescale_guided_eps
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.engine import MkdEngine, NetConfig, sample_log_rows, unipc_table
from makeupdiffuse_amd.unipc import UniPCSampler
from oracle import nets, sampler, vae

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))

# Limits of the two measured comparisons (DESIGN.md §2 convention: 3 x the measured distance, cosine >= 0.99).  Measured on the MI355X,
# small nets, 10 steps, batch 2, 8x8 latents (rel-L2; plain / guidance 9):
#   order 2 with the corrector off vs mkd_sample_dpmpp order 2 on the same context: measured 0, graph and eager alike.  On this grid
#     the two host tables round to the same floats (1/alpha, sigma, a_p = c_x, p_0 = c_0, p_1 = c_1: checked on the CPU in
#     tests/test_unipc_host.py) and both kernels sum a x + c_0 m_k + c_1 m_{k-1} in that order with explicit fmas, so the two loops
#     give the same bits and 3 x 0 allows nothing else
#   order 2 with the corrector on vs the float64 restatement (tests/unipc_ref.py) driven by the fp32 oracle nets
MEASURED_NOCOR = {1.0: 0.0, 9.0: 0.0}
MEASURED_TRAJ = {1.0: 3.1487e-3, 9.0: 2.1622e-2}
COS_CAP = 0.99
# The trajectory budget the DPM-Solver++ tests' MEASURED_TRAJ documents: a multi-step latent keeps cosine >= 0.99 to the
# oracle's.  For two latents of about one norm rel-L2^2 = 2 (1 - cos), so a rel-L2 limit is inside that budget while it is below
TRAJ_BUDGET = math.sqrt(2.0 * (1.0 - COS_CAP))          # 0.1414


def limit(measured):
    return 3.0 * measured


def metrics(out, ref):
    out = out.float().cpu(); ref = ref.float().cpu()
    assert torch.isfinite(out).all(), 'non-finite output'
    return ((out - ref).norm() / ref.norm()).item(), F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()


@pytest.fixture(scope='module')
def mm():
    sd = nets.init_state_dict(OCFG, seed=31)
    vcfg = vae.VaeConfig(z_channels=4, embed_dim=4, ch=32, ch_mult=(1, 2, 2, 2), num_res_blocks=1, out_ch=3)
    m = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                         unet_config={'params': dict(NET, out_channels=4)},
                         first_stage_config={'params': {'embed_dim': 4, 'ddconfig': dict(VSMALL)}}, first_stage_encoder=True,
                         ddim_steps=10, unconditional_guidance_scale=9)
    m.load_state_dict({**sd, **vae.init_state_dict(vcfg, seed=32), **enc_ref.init_state_dict(vcfg, seed=33)})
    m.cuda(0)
    g = torch.Generator().manual_seed(34)
    m.uncond_embedding = torch.randn(1, 77, 64, generator=g)
    m.save_images = False
    return m, sd


def small_engine(sd):
    eng = MkdEngine(NetConfig(hint_channels=6, model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2,
                              context_dim=64, hint_widths=tuple(HINT_WIDTHS)))
    eng.load_state_dict(sd)
    return eng


def inputs(B=2, res=64, seed=35):
    g = torch.Generator().manual_seed(seed)
    h = res // 8
    return dict(hint=torch.rand(B, 6, res, res, generator=g).to(DEV), ctx=torch.randn(B, 77, 64, generator=g).to(DEV),
                uctx=torch.randn(B, 77, 64, generator=g).to(DEV), x_T=torch.randn(B, 4, h, h, generator=g).to(DEV),
                x0=torch.randn(B, 4, h, h, generator=g).to(DEV),
                mask=(torch.rand(B, 1, h, h, generator=g) > 0.5).float().to(DEV))


def prepare(eng, I, cfg):
    if cfg == 1.0:
        eng.prepare(I['hint'], I['ctx'])
    else:
        eng.prepare(torch.cat([I['hint'], I['hint']]), torch.cat([I['uctx'], I['ctx']]))


def conds(I, scale):
    c = {'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]}
    uc = {'c_crossattn': [I['uctx']], 'c_concat': [I['hint']]} if scale != 1.0 else None
    return c, uc


def ddim_tables(S):
    sch = sampler.Schedule().make_ddim(S)
    return [int(t) for t in sch.ddim_timesteps], sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas


# ---- 1. the step kernel ----------------------------------------------------------------------------------------------------------
# fp32 roundings per output of one element (c of the bound c 2^-24 sum |terms|; unipc_ref.step_fp64 gives the sums, in which the
# magnitude sum of an fp32 intermediate stands in for it where an output is built on it):
#   e    guided: the difference e_c - e_u and the fma                                            2   (plain: 0)
#   m0   = fma(-sigma, e, x) * (1 / alpha): the fma, the product                                +2 = 4
#   xc   = a_c xcp, then one fma each for q_0 m0, q_1 m1, q_2 m2, q_3 m3                        +5 = 9   (no corrector: xc = x, 0)
#   x'   = a_p xc, then one fma each for p_0 m0, p_1 m1, p_2 m2                                 +4 = 13
# The rescaled eps (k non-null) multiplies e by the fp32 factor k[b]: one more rounding in e and one in k itself, +2 on every count.
C_M0, C_XC, C_X = 4, 9, 13


def call_step(lib, x, xcp, e_c, e_u, scale, k, m1, m2, m3, outs):
    cor = k[2] != 0
    return lib.mkd_unipc_step(P(x), P(xcp) if cor else None, P(e_c), P(e_u), scale, (C.c_float * 12)(*k.tolist()),
                              P(m1) if (cor and k[4] != 0) or k[9] != 0 else None, P(m2) if (cor and k[5] != 0) or k[10] != 0 else None,
                              P(m3) if cor and k[6] != 0 else None, P(outs[0]), P(outs[1]), P(outs[2]), x.numel(), None)


@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('corrector', [True, False])
@pytest.mark.parametrize('n', [4 * 8 * 8 * 2, 1003, 4099])          # 16-byte form, and two sizes that are no multiple of 4
def test_step_kernel_against_fp64(guided, corrector, n):
    """All three outputs per element: |err| <= c 2^-24 sum |terms| with c = 4 (m0), 9 (xc), 13 (x'), the counts above.  Executed steps
    k = 0, 1, 2, 3 and the last of an order-3 table: no history; x^c and m1; then m2; then m3 (every null / non-null pattern)."""
    lib = L()
    _, a, ap = dref.grid(20)
    coef, so = unipc_table(a, ap, 3, True, corrector)
    g = torch.Generator().manual_seed(1000 * int(corrector) + n % 97 + int(guided))
    hist_used = set()
    for i in (19, 18, 17, 16, 9, 0):
        k = coef[i]
        assert so[i] == min(3, 20 - i)
        cor = k[2] != 0
        assert cor == (corrector and i < 19)
        hist_used.add((cor, bool(k[4] != 0 or k[9] != 0), bool(k[5] != 0 or k[10] != 0), bool(k[6] != 0)))
        x, xcp, e_c, e_u, m1, m2, m3 = (torch.randn(n, generator=g).to(DEV) for _ in range(7))
        scale = 9.0 if guided else 1.0
        outs = [torch.full((n,), float('nan'), device=DEV) for _ in range(3)]
        assert call_step(lib, x, xcp, e_c, e_u if guided else None, scale, k, m1, m2, m3, outs) == 0
        sync()
        refs, mags = uref.step_fp64(x.cpu(), xcp.cpu(), e_c.cpu(), e_u.cpu() if guided else None, scale, k, m1.cpu(), m2.cpu(), m3.cpu())
        for name, out, ref, mag, c in zip(('x_next', 'xc', 'm0'), outs, refs, mags, (C_X, C_XC, C_M0)):
            err = (out.cpu().double() - ref).abs()
            worst = (err / mag).max().item() / 2 ** -24
            print(f'[unipc step] corrector {cor} guided {guided} n {n} entry {i} {name}: max err / (2^-24 mag) x {worst:.2f} (bound {c})')
            assert (err <= c * 2 ** -24 * mag).all(), f'{name}: {worst:.2f} x 2^-24'
        if not cor:
            assert torch.equal(outs[1], x)                     # no corrector: x^c_k is x~_k itself
        # in place (x_next = x, xc_out = xc_prev) gives the same bits
        xi, ci = x.clone(), xcp.clone()
        m0b = torch.empty_like(x)
        assert call_step(lib, xi, ci, e_c, e_u if guided else None, scale, k, m1, m2, m3, [xi, ci, m0b]) == 0
        sync()
        assert torch.equal(xi, outs[0]) and torch.equal(ci, outs[1]) and torch.equal(m0b, outs[2])
    if corrector:
        assert hist_used == {(False, False, False, False), (True, True, False, False), (True, True, True, False), (True, True, True, True)}
    else:
        assert hist_used == {(False, False, False, False), (False, True, False, False), (False, True, True, False)}


def test_step_refuses_a_coefficient_without_its_tensor():
    lib = L()
    _, a, ap = dref.grid(20)
    coef, _ = unipc_table(a, ap, 3, True, True)
    n = 64
    x, xcp, e, m1, m2, m3, o0, o1, o2 = (torch.zeros(n, device=DEV) for _ in range(9))
    k = (C.c_float * 12)(*coef[0].tolist())
    ok = [P(x), P(xcp), P(e), None, 1.0, k, P(m1), P(m2), P(m3), P(o0), P(o1), P(o2), n, None]
    assert lib.mkd_unipc_step(*ok) == 0
    for hole in (0, 1, 2, 5, 6, 7, 8, 9, 10, 11):                # x, x^c_{k-1}, eps_c, the row, m1, m2, m3, the three outputs
        args = list(ok); args[hole] = None
        assert lib.mkd_unipc_step(*args) == -1, hole
    args = list(ok); args[12] = 0
    assert lib.mkd_unipc_step(*args) == -1
    kf = torch.ones(2, device=DEV)
    ex = [P(x), P(xcp), P(e), None, 9.0, k, P(m1), P(m2), P(m3), P(kf), 32, P(o0), P(o1), P(o2), n, None]
    assert lib.mkd_unipc_step_ex(*ex) == -1                      # a factor without eps_u
    ex[3] = P(e); ex[10] = 48
    assert lib.mkd_unipc_step_ex(*ex) == -1                      # n_per_sample does not divide n
    ex[10] = 32
    assert lib.mkd_unipc_step_ex(*ex) == 0
    sync()


def test_vector_and_scalar_forms_give_the_same_bits():
    """the same elements through the 16-byte form (aligned, n % 4 == 0) and the scalar form (views 4 bytes off): one arithmetic"""
    lib = L()
    _, a, ap = dref.grid(20)
    coef, _ = unipc_table(a, ap, 3, True, True)
    k = coef[0]
    g = torch.Generator().manual_seed(7)
    n = 2048
    bufs = [torch.randn(n + 1, generator=g).to(DEV) for _ in range(7)]
    for e_u_on in (True, False):
        res = []
        for aligned in (True, False):
            x, xcp, e_c, e_u, m1, m2, m3 = (b[1:].clone() if aligned else b[1:] for b in bufs)
            assert all((t.data_ptr() % 16 == 0) == aligned for t in (x, xcp, e_c, e_u, m1, m2, m3))
            outs = [torch.empty(n + 1, device=DEV)[1:] for _ in range(3)]
            if aligned:
                outs = [o.clone() for o in outs]
            assert call_step(lib, x, xcp, e_c, e_u if e_u_on else None, 9.0, k, m1, m2, m3, outs) == 0
            sync()
            res.append([o.clone() for o in outs])
        for u, v in zip(*res):
            assert torch.equal(u, v)


def test_rescaled_step_against_rescale_guided_eps(mm):
    """the step with the per-sample rescale factors (mkd_unipc_step_ex through MkdEngine.unipc_step) against float64 with
    e = rescale_guided_eps(e_c, e_u, s, phi): the counts above + 2"""
    m, _ = mm
    eng = m.engine
    _, a, ap = dref.grid(20)
    coef, _ = unipc_table(a, ap, 3, True, True)
    g = torch.Generator().manual_seed(11)
    x, xcp, e_c, e_u, m1, m2, m3 = (torch.randn(2, 4, 8, 8, generator=g).to(DEV) for _ in range(7))
    k = coef[3]
    outs = eng.unipc_step(x, xcp, e_c, e_u, 9.0, k, m1, m2, m3, guidance_rescale=0.7)
    sync()
    ec64, eu64 = e_c.cpu().double(), e_u.cpu().double()
    e = rescale_guided_eps(ec64, eu64, 9.0, 0.7)
    gd = eu64 + 9.0 * (ec64 - eu64)
    kf = 0.7 * ec64.std(dim=(1, 2, 3), keepdim=True) / gd.std(dim=(1, 2, 3), keepdim=True) + 0.3
    assert torch.allclose(e, gd * kf, rtol=1e-12, atol=0)
    emag = (eu64.abs() + 9.0 * (ec64 - eu64).abs()) * kf
    refs, mags = uref.step_fp64(x.cpu(), xcp.cpu(), e, None, 1.0, k, m1.cpu(), m2.cpu(), m3.cpu(), e_mag=emag)
    for name, out, ref, mag, c in zip(('x_next', 'xc', 'm0'), outs, refs, mags, (C_X + 2, C_XC + 2, C_M0 + 2)):
        err = (out.cpu().double() - ref).abs()
        print(f'[unipc step] rescaled {name}: max err / (2^-24 mag) x {(err / mag).max().item() / 2 ** -24:.2f} (bound {c})')
        assert (err <= c * 2 ** -24 * mag).all(), name
    plain = eng.unipc_step(x, xcp, e_c, e_u, 9.0, k, m1, m2, m3)
    assert metrics(outs[0], plain[0])[0] > 1e-2                  # (the factor is not 1: another latent)


# ---- 2. one arithmetic: every loop form gives the per-step class loop's bits --------------------------------------------------
@pytest.mark.parametrize('corrector', [True, False])
@pytest.mark.parametrize('scale', [1.0, 9.0])
@pytest.mark.parametrize('order', [1, 2, 3])
def test_in_library_loops_equal_the_step_loop(mm, order, scale, corrector):
    m, _ = mm
    I = inputs()
    c, uc = conds(I, scale)
    smp = UniPCSampler(m)
    kw = dict(unconditional_guidance_scale=scale, unconditional_conditioning=uc, order=order, corrector=corrector)
    smp.make_schedule(10)
    for poisoned in (False, True):
        if poisoned:
            m.engine.debug_poison()
        outs = {}
        outs['graph'] = smp.decode(I['x_T'], c, 7, **kw)          # 7 steps: one 5-step graph + two single-step replays
        m.sample_use_graph = False
        try:
            outs['eager'] = smp.decode(I['x_T'], c, 7, **kw)
        finally:
            m.sample_use_graph = True
        outs['steps'] = smp.decode(I['x_T'], c, 7, callback=lambda k: None, **kw)
        for k in ('eager', 'steps'):
            assert torch.equal(outs[k], outs['graph']), f'{k} != graph (order {order}, scale {scale}, corrector {corrector}, poisoned {poisoned})'
    full, _ = smp.sample(10, 2, (4, 8, 8), conditioning=c, x_T=I['x_T'], **kw)
    full_steps, _ = smp.sample(10, 2, (4, 8, 8), conditioning=c, x_T=I['x_T'], callback=lambda k: None, **kw)
    assert torch.equal(full, full_steps)
    if corrector:          # (the corrector is not a no-op: another latent than the predictor alone)
        other, _ = smp.sample(10, 2, (4, 8, 8), conditioning=c, x_T=I['x_T'], **dict(kw, corrector=False))
        assert metrics(full, other)[0] > 1e-3


def test_linear_graph_segments_equal_the_eager_loop(monkeypatch):
    monkeypatch.setenv('MKD_GRAPH_MODE', '2')
    eng = small_engine(nets.init_state_dict(OCFG, seed=31))
    I = inputs()
    ts, a, ap = dref.grid(7)
    args = ([int(t) for t in ts], a, ap)
    dd = ddim_tables(10)
    for cfg in (1.0, 9.0):
        prepare(eng, I, cfg)
        for order, cor in ((1, True), (2, True), (2, False), (3, True), (3, False)):
            e = eng.sample_unipc(I['x_T'], *args, order=order, corrector=cor, cfg_scale=cfg, use_graph=False)
            s1 = eng.sample_unipc(I['x_T'], *args, order=order, corrector=cor, cfg_scale=cfg, use_graph=True)
            d = eng.sample(I['x_T'], *dd, cfg_scale=cfg, use_graph=True)              # a DDIM call between two UniPC calls: re-captures
            eng.debug_poison()
            s2 = eng.sample_unipc(I['x_T'], *args, order=order, corrector=cor, cfg_scale=cfg, use_graph=True)
            assert torch.equal(e, s1) and torch.equal(e, s2), f'segments != eager (cfg {cfg}, order {order}, corrector {cor})'
            assert torch.equal(d, eng.sample(I['x_T'], *dd, cfg_scale=cfg, use_graph=False))
    eng.close()


# ---- 3. the corrector-free order 2 against the DPM-Solver++ loop ---------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 9.0])
def test_order_two_without_corrector_against_the_dpmpp_loop(mm, scale):
    """The predictor alone at order 2 is the DPM-Solver++ 2M step: limit 3 x the measured rel-L2, cosine >= 0.99.  Measured: 0, the
    same bits (MEASURED_NOCOR above says why), so this is an equality."""
    m, _ = mm
    eng = m.engine
    I = inputs()
    prepare(eng, I, scale)
    m.reset_conditioning_cache()
    ts, a, ap, _ = ddim_tables(10)
    for g in (True, False):
        dpm = eng.sample_dpmpp(I['x_T'], ts, a, ap, order=2, cfg_scale=scale, use_graph=g)
        uni = eng.sample_unipc(I['x_T'], ts, a, ap, order=2, corrector=False, cfg_scale=scale, use_graph=g)
        r, cs = metrics(uni, dpm)
        print(f'[parity] UniPC order 2, corrector off vs DPM-Solver++ order 2 loop, 10 steps, scale {scale}, graph {g}: rel-L2 {r:.4e} cos {cs:.8f}')
        assert cs >= COS_CAP and r <= limit(MEASURED_NOCOR[scale])


# ---- 4. trajectory against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 9.0])
def test_order_two_trajectory_vs_oracle(mm, scale):
    m, sd = mm
    I = inputs(seed=52)
    c, uc = conds(I, scale)
    out, _ = UniPCSampler(m).sample(10, 2, (4, 8, 8), conditioning=c, x_T=I['x_T'], order=2, corrector=True,
                                    unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    sch = sampler.Schedule().make_ddim(10)
    cpu = lambda d: None if d is None else {k: [t.cpu() for t in v] for k, v in d.items()}
    ref = uref.unipc(sampler.make_eps_fn(sd, OCFG), sch.ddim_timesteps, sch.ddim_alphas.numpy(), sch.ddim_alphas_prev.numpy(),
                     I['x_T'].cpu(), cpu(c), order=2, corrector=True, scale=scale, uc=cpu(uc))
    r, cs = metrics(out, ref)
    print(f'[parity] UniPC order 2 with the corrector, 10-step latent vs oracle, scale {scale}: rel-L2 {r:.4e} cos {cs:.6f}')
    assert limit(MEASURED_TRAJ[scale]) <= TRAJ_BUDGET
    assert cs >= COS_CAP and r <= limit(MEASURED_TRAJ[scale])


# ---- 5. trace and guidance rescale ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order,corrector', [(2, True), (3, True), (2, False)])
def test_trace_and_rescale_equal_the_step_loop(mm, order, corrector):
    """the in-library loop's trace rows (x_inter: the predicted latents; pred_x0: m_k) and its rescaled guidance (phi = 0.7), graph
    and eager, against the per-step class loop, which takes each step's intermediates from mkd_unipc_step / mkd_unipc_step_ex"""
    m, _ = mm
    I = inputs()
    S = 10
    for scale, phi in ((1.0, 0.0), (9.0, 0.0), (9.0, 0.7)):
        c, uc = conds(I, scale)
        for Lt in (1, 3, 100):
            kw = dict(conditioning=c, x_T=I['x_T'], order=order, corrector=corrector, unconditional_guidance_scale=scale,
                      unconditional_conditioning=uc, log_every_t=Lt, guidance_rescale=phi)
            lat_s, inter_s = UniPCSampler(m).sample(S, 2, (4, 8, 8), callback=lambda k: None, **kw)
            for graph in ((True, False) if Lt == 3 else (True,)):
                m.sample_use_graph = graph
                try:
                    lat, inter = UniPCSampler(m).sample(S, 2, (4, 8, 8), **kw)
                finally:
                    m.sample_use_graph = True
                what = f'order {order} corrector {corrector} L {Lt} scale {scale} phi {phi} graph {graph}'
                assert torch.equal(lat, lat_s), f'latent: {what}'
                for key in ('x_inter', 'pred_x0'):
                    assert len(inter[key]) == len(inter_s[key]) == 1 + sample_log_rows(S, Lt), f'{key}: {what}'
                    for j, (a_, b_) in enumerate(zip(inter[key], inter_s[key])):
                        assert torch.equal(a_, b_), f'{key}[{j}]: {what}'
                assert torch.equal(inter['x_inter'][-1], lat)
    c, uc = conds(I, 9.0)
    kw = dict(conditioning=c, x_T=I['x_T'], order=order, corrector=corrector, unconditional_guidance_scale=9.0, unconditional_conditioning=uc)
    plain, _ = UniPCSampler(m).sample(S, 2, (4, 8, 8), **kw)
    resc, _ = UniPCSampler(m).sample(S, 2, (4, 8, 8), guidance_rescale=0.7, **kw)
    assert metrics(resc, plain)[0] > 1e-2                        # (the rescale is engaged)


# ---- 6. shared state -------------------------------------------------------------------------------------------------------------
def test_ddim_unipc_dpmpp_unipc_on_one_context(mm):
    m, _ = mm
    eng = m.engine
    I = inputs()
    ts, a, ap, s1 = ddim_tables(10)
    for scale in (1.0, 9.0):
        prepare(eng, I, scale)
        m.reset_conditioning_cache()
        for g in (True, False):
            d0 = eng.sample(I['x_T'], ts, a, ap, s1, cfg_scale=scale, use_graph=g)
            u0 = eng.sample_unipc(I['x_T'], ts, a, ap, order=3, cfg_scale=scale, use_graph=g)
            p0 = eng.sample_dpmpp(I['x_T'], ts, a, ap, order=3, cfg_scale=scale, use_graph=g)
            u1 = eng.sample_unipc(I['x_T'], ts, a, ap, order=3, cfg_scale=scale, use_graph=g)
            d1 = eng.sample(I['x_T'], ts, a, ap, s1, cfg_scale=scale, use_graph=g)
            p1 = eng.sample_dpmpp(I['x_T'], ts, a, ap, order=3, cfg_scale=scale, use_graph=g)
            assert torch.equal(u0, u1), f'UniPC changed after a DPM-Solver++ call (scale {scale}, graph {g})'
            assert torch.equal(d0, d1) and torch.equal(p0, p1), f'DDIM / DPM-Solver++ changed after a UniPC call (scale {scale}, graph {g})'
            assert not torch.equal(u0, d0) and not torch.equal(u0, p0)


def test_ring_regrowth_batch_2_4_2():
    eng = small_engine(nets.init_state_dict(OCFG, seed=31))          # a fresh context: its ring starts at batch 2
    I4 = inputs(B=4, seed=36)
    I2 = {k: v[:2].contiguous() for k, v in I4.items()}
    ts, a, ap, _ = ddim_tables(10)
    run = lambda I, g: eng.sample_unipc(I['x_T'], ts, a, ap, order=3, use_graph=g)
    for g in (True, False):
        prepare(eng, I2, 1.0); first = run(I2, g)
        prepare(eng, I4, 1.0); big = run(I4, g)
        prepare(eng, I2, 1.0); again = run(I2, g)
        assert torch.equal(first, again), f'batch 2 after batch 4 changed (graph {g})'
        assert metrics(big[:2], first)[0] <= 2e-2                      # the same samples inside the larger batch (other GEMM shapes)
    # a DPM-Solver++ call first (a three-plane ring), then UniPC at the same batch (five planes): the ring grows
    eng2 = small_engine(nets.init_state_dict(OCFG, seed=31))
    prepare(eng2, I2, 1.0)
    eng2.sample_dpmpp(I2['x_T'], ts, a, ap, order=3, use_graph=True)
    assert torch.equal(eng2.sample_unipc(I2['x_T'], ts, a, ap, order=3, use_graph=True), first)
    eng.close(); eng2.close()


# ---- 7. launch count -------------------------------------------------------------------------------------------------------------
def test_step_launch_count_is_ddims(mm):
    """mkd_step_launches_ex is what the loop enqueues per step whichever solver ends it (setup + evaluation + ONE update kernel): the
    numbers do not move across DDIM and UniPC calls - the corrector, the predictor, the history ring and x^c are the update kernel's."""
    m, _ = mm
    eng = m.engine
    I = inputs()
    ts, a, ap, s1 = ddim_tables(10)
    for scale in (1.0, 9.0):
        prepare(eng, I, scale)
        m.reset_conditioning_cache()
        eng.sample(I['x_T'], ts, a, ap, s1, cfg_scale=scale, use_graph=True)
        before = [eng.step_launches(g, c) for g in (True, False) for c in (False, True)]
        eng.sample_unipc(I['x_T'], ts, a, ap, order=3, cfg_scale=scale, use_graph=True)
        eng.sample_unipc(I['x_T'], ts, a, ap, order=3, cfg_scale=scale, use_graph=False)
        assert [eng.step_launches(g, c) for g in (True, False) for c in (False, True)] == before


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_masked_call_is_refused_and_the_context_stays_usable(mm):
    m, _ = mm
    eng = m.engine
    I = inputs()
    prepare(eng, I, 1.0)
    m.reset_conditioning_cache()
    ts, a, ap, _ = ddim_tables(10)
    before = eng.sample_unipc(I['x_T'], ts, a, ap, use_graph=True)
    sch = sampler.Schedule()
    q = dict(x0=I['x0'], mask=I['mask'], q_sqrt_ac=[float(sch.alphas_cumprod[t]) ** 0.5 for t in ts],
             q_sqrt_1m_ac=[float(1.0 - sch.alphas_cumprod[t]) ** 0.5 for t in ts], q_noise=torch.randn(10, 2, 4, 8, 8, device=DEV))
    for g in (True, False):
        with pytest.raises(mlib.MkdError, match=r'\(-4\)'):
            eng.sample_unipc(I['x_T'], ts, a, ap, use_graph=g, **q)
    assert torch.equal(eng.sample_unipc(I['x_T'], ts, a, ap, use_graph=True), before)
    c, _ = conds(I, 1.0)
    with pytest.raises(NotImplementedError):
        UniPCSampler(m).sample(10, 2, (4, 8, 8), conditioning=c, x_T=I['x_T'], mask=I['mask'], x0=I['x0'])
    # a table that is not contiguous, through the loop entry: MKD_ERR_ARG
    gap = np.asarray(ap, dtype=np.float32).copy(); gap[5] = 0.5 * (gap[5] + gap[4])
    with pytest.raises(mlib.MkdError, match=r'\(-1\)'):
        eng.sample_unipc(I['x_T'], ts, a, gap, use_graph=True)
    assert torch.equal(eng.sample_unipc(I['x_T'], ts, a, ap, use_graph=False), before)


# ---- 9. the model surface ----------------------------------------------------------------------------------------------------------
def test_log_results_with_the_unipc_sampler(mm):
    m, _ = mm
    g = torch.Generator().manual_seed(70)
    B = 2
    batch = {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g),
             'txt_emb': torch.randn(B, 77, 64, generator=g)}
    x_T = torch.randn(B, 4, 8, 8, generator=g).to(DEV)
    base = m.log_results(batch, 0, x_T=x_T)
    m.sampler, m.solver_order = 'dpmpp', 2
    try:
        dpm = m.log_results(batch, 0, x_T=x_T)
        m.sampler = 'unipc'
        log = m.log_results(batch, 0, x_T=x_T)
        m.unipc_corrector = False
        nocor = m.log_results(batch, 0, x_T=x_T)
        m.unipc_corrector = True
        m.fix_background = True
        with pytest.raises(NotImplementedError):
            m.log_results(dict(batch, nonmakeup_seg=torch.zeros(B, 64, 64, dtype=torch.uint8)), 0, x_T=x_T)
    finally:
        m.sampler, m.unipc_corrector, m.fix_background = 'ddim', True, False
    assert set(log) == set(base)
    for k in base:
        assert tuple(log[k].shape) == tuple(base[k].shape), k
    for k in ('samples_latent', 'samples_cfg_scale_9.00_latent', 'samples', 'samples_cfg_scale_9.00'):
        assert torch.isfinite(log[k]).all() and metrics(log[k], base[k])[0] > 1e-4, k       # both passes ran on the other solver
        assert metrics(log[k], dpm[k])[0] > 1e-4 and metrics(log[k], nocor[k])[0] > 1e-4, k  # ... and on this one, with its corrector
    again = m.log_results(batch, 0, x_T=x_T)
    assert torch.equal(again['samples_latent'], base['samples_latent'])                       # the default path is untouched
    m2 = TestDiffuseModel(control_stage_config={'params': dict(NET, hint_channels=6, hint_widths=HINT_WIDTHS)},
                          unet_config={'params': dict(NET, out_channels=4)}, sampler='unipc', solver_order=3, unipc_corrector=False)
    assert (m2.sampler, m2.solver_order, m2.unipc_corrector) == ('unipc', 3, False)


def test_runs_test_py_with_the_unipc_sampler(tmp_path):
    from PIL import Image
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--pairs', '2', '--batch-size', '2', '--res', '64',
                        '--ddim-steps', '4', '--sampler', 'unipc', '--solver-order', '2', '--seed', '5', '--out', str(out)],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    root = out / 'makeupdiffuse_mi355x'
    names = sorted(os.listdir(root))
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'samples_0000.png', 'samples_cfg_scale_9.00_0000.png'], names
    g = np.asarray(Image.open(root / 'samples_0000.png'))
    assert g.shape == (64 + 4, 2 * 66 + 2, 3) and g.std() > 1.0
    lat = torch.load(out / 'latents_0000.pt')
    assert tuple(lat['samples_latent'].shape) == (2, 4, 8, 8) and torch.isfinite(lat['samples_latent']).all()
