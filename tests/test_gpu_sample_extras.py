"""-m gpu: the in-library sampling loop's extras on the device.  The guidance-rescale factor kernel and the step kernels with a factor
against float64, every loop form (graph replay, linear graph segments, eager) against the per-step class loop bit for bit with the
intermediates trace and with the rescale, the state traced / rescaled and plain calls share on one context, the step-launch count,
the argument checks, the rescaled trajectory against the oracle nets, and the model surface (denoise rows, runs/test.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dpm_solver_ref as dref
import sample_extras_ref as xref
import vae_encoder_ref as enc_ref
from gpu_util import DEV, L, P, sync
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd.ddim import DDIMSampler
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler
from makeupdiffuse_amd.engine import MkdEngine, NetConfig, dpmpp_table, sample_log_rows, unipc_table
from oracle import nets, sampler, vae

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
           context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
HINT_WIDTHS = [16, 16, 32, 32, 32, 32, 64]
VSMALL = dict(z_channels=4, ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=1, out_ch=3, attn_resolutions=[])
OCFG = nets.NetConfig(model_channels=64, channel_mult=(1, 2), attention_resolutions=(1, 2), num_heads=2, context_dim=64,
                      hint_widths=tuple(HINT_WIDTHS))
PHI = 0.7

# Limit of the rescaled trajectory (DESIGN.md section 2 convention: 3 x the distance measured on the MI355X, cosine >= 0.99): small nets,
# 10 steps, batch 2, 8x8 latents, guidance 9, phi 0.7, the device loop against the restated loop over the fp32 oracle nets (rel-L2)
MEASURED_RESCALED = {'ddim': 1.6708e-2, 'dpm2': 1.5472e-2}
COS_CAP = 0.99


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
                         ddim_steps=8, unconditional_guidance_scale=9)
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


@pytest.fixture(scope='module')
def engines():
    """(a context with the default single-graph replay, one whose replay runs as per-stream linear segments)"""
    sd = nets.init_state_dict(OCFG, seed=31)
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


# ---- 1. the factor kernel ------------------------------------------------------------------------------------------------------
def factor_inputs(kind, B, n, g):
    e_c, e_u = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    if kind == 'offset':                     # mean 100, std 1: sum(v^2) - sum(v)^2 / n cancels four digits
        e_c, e_u = e_c + 100.0, e_u + 100.0
    elif kind == 'spread':                   # another std per sample: a batch-wide reduction gives one factor for all
        e_c = e_c * torch.tensor([1.0, 1e-3, 50.0])[:B].view(B, 1)
    elif kind == 'equal':
        e_u = e_c.clone()
    elif kind == 'const':
        e_c = torch.full((B, n), 0.3) * torch.tensor([1.0, -7.1, 100.1])[:B].view(B, 1)
        e_u = e_c.clone()
    return e_c.contiguous(), e_u.contiguous()


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('n', [140, 256, 1003, 4096, 16388])      # fewer elements than threads, one each, ragged, the 256^2 latent, past the 512^2 one
def test_factor_kernel_against_fp64(B, n):
    """|k - k_ref| <= 2 * 2^-24 |k_ref| with k_ref the float64 two-pass statement over the fp32 g = fmaf(s, e_c - e_u, e_u).
    The kernel rounds ONCE, k (double) -> float: 2^-24 relative.  Everything before it is fp64: the sums have at most
    n / 256 + 6 + 3 <= 74 additions each (relative 74 * 2^-53 of sum |v^2|), and var = sum(v^2) - sum(v)^2 / n amplifies that by
    sum(v^2) / (n var) <= 1e4 + 1 here (mean 100, std 1): 74 * 1.1e-16 * 1e4 = 8e-11, a 1e-3 part of 2^-24.  c = 2 covers both
    with room for the reference's own fp64 rounding.  e_c == e_u gives k = 1 exactly (the ratio of two equal sums), a constant g
    gives exactly 1 too (var(g) is not above the rounding error of its sums, 4 n 2^-52 sum(g^2): counted as zero) and stays finite."""
    lib = L()
    g = torch.Generator().manual_seed(1000 * B + n)
    for kind in ('randn', 'offset', 'spread', 'equal', 'const'):
        e_c, e_u = factor_inputs(kind, B, n, g)
        dc, du = e_c.to(DEV), e_u.to(DEV)
        for scale, phi in ((9.0, PHI), (9.0, 1.0), (2.5, 0.3)):
            k = torch.full((B,), float('nan'), device=DEV)
            assert lib.mkd_cfg_rescale_factor(P(dc), P(du), scale, phi, B, n, P(k), None) == 0
            k2 = torch.full((B,), float('nan'), device=DEV)
            assert lib.mkd_cfg_rescale_factor(P(dc), P(du), scale, phi, B, n, P(k2), None) == 0
            sync()
            assert torch.equal(k, k2), f'{kind}: two runs differ'
            kd = k.cpu().double()
            assert torch.isfinite(kd).all(), f'{kind}: non-finite factor {kd.tolist()}'
            if kind in ('equal', 'const'):
                assert (kd == 1.0).all(), f'{kind}: {kd.tolist()}'
                continue
            ref = xref.rescale_factor64(e_c, e_u, scale, float(np.float32(phi)), g=xref.guided_f32(e_c, e_u, scale))
            worst = ((kd - ref).abs() / ref.abs()).max().item() / 2 ** -24
            print(f'[rescale factor] {kind} B {B} n {n} s {scale} phi {phi}: k {kd.tolist()} err {worst:.3f} x 2^-24')
            assert ((kd - ref).abs() <= 2 * 2 ** -24 * ref.abs()).all(), f'{kind}: {worst:.2f} x 2^-24'
            if kind == 'spread' and B == 3:
                assert kd.max() - kd.min() > 1e-2              # per sample
    bad = torch.zeros(4, device=DEV)
    assert lib.mkd_cfg_rescale_factor(P(bad), P(bad), 9.0, 1.5, 1, 4, P(bad), None) == -1
    assert lib.mkd_cfg_rescale_factor(P(bad), None, 9.0, 0.5, 1, 4, P(bad), None) == -1
    assert lib.mkd_cfg_rescale_factor(P(bad), P(bad), 9.0, 0.5, 0, 4, P(bad), None) == -1


# ---- 2. the step kernels with a factor --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('n,per', [(4 * 8 * 8 * 2, 256), (1003, 59), (4099, 4099)])      # 16-byte form, two sizes that are no multiple of 4
def test_dpm_step_kernel_with_factor_against_fp64(order, n, per):
    """test_step_kernel_against_fp64's bound plus the one rounding of e = g * k: |err| <= 9 * 2^-24 * (|c_x x| + sum |c_j m_j|), m0
    against (|x| + sigma k (|e_u| + |s (e_c - e_u)|)) / alpha.  k is the device factor kernel's, read back."""
    lib = L()
    _, a, ap = dref.grid(20)
    coef, so = dpmpp_table(a, ap, order, True)
    g = torch.Generator().manual_seed(300 * order + n % 97)
    B = n // per
    for i in (19, 18, 10, 0):
        kc = coef[i]
        x, e_c, e_u, m1, m2 = (torch.randn(n, generator=g).to(DEV) for _ in range(5))
        kf = torch.empty(B, device=DEV)
        assert lib.mkd_cfg_rescale_factor(P(e_c), P(e_u), 9.0, PHI, B, per, P(kf), None) == 0
        xp = torch.full((n,), float('nan'), device=DEV); m0 = torch.full((n,), float('nan'), device=DEV)
        args = (P(x), P(e_c), P(e_u), 9.0, (C.c_float * 6)(*kc.tolist()), P(m1) if kc[4] != 0 else None, P(m2) if kc[5] != 0 else None)
        assert lib.mkd_dpmpp_step_ex(*args, P(kf), per, P(xp), P(m0), n, None) == 0
        sync()
        kk = kf.cpu().double().repeat_interleave(per)
        ed = (e_u.cpu().double() + 9.0 * (e_c.cpu().double() - e_u.cpu().double())) * kk
        ref, m0_ref, mag, _ = dref.step_fp64(x.cpu(), ed, None, 1.0, kc, m1.cpu(), m2.cpu())
        k6 = [float(np.float32(v)) for v in kc]
        m0_mag = (x.cpu().double().abs() + k6[1] * kk * (e_u.cpu().double().abs() + 9.0 * (e_c.cpu().double() - e_u.cpu().double()).abs())) * k6[0]
        err, err0 = (xp.cpu().double() - ref).abs(), (m0.cpu().double() - m0_ref).abs()
        print(f'[dpm step + k] order {so[i]} n {n} entry {i}: x {(err / mag).max().item() / 2 ** -24:.2f}, m0 {(err0 / m0_mag).max().item() / 2 ** -24:.2f} x 2^-24')
        assert (err <= 9 * 2 ** -24 * mag).all() and (err0 <= 9 * 2 ** -24 * m0_mag).all()
        # k == NULL is mkd_dpmpp_step, bit for bit; the factor does change the result
        p1 = torch.empty_like(x); q1 = torch.empty_like(x); p2 = torch.empty_like(x); q2 = torch.empty_like(x)
        assert lib.mkd_dpmpp_step_ex(*args, None, 0, P(p1), P(q1), n, None) == 0
        assert lib.mkd_dpmpp_step(*args, P(p2), P(q2), n, None) == 0
        sync()
        assert torch.equal(p1, p2) and torch.equal(q1, q2) and not torch.equal(p1, xp)
    kf = torch.ones(B, device=DEV)
    assert lib.mkd_dpmpp_step_ex(*args[:2], None, *args[3:], P(kf), per, P(xp), P(m0), n, None) == -1        # k without eps_u
    assert lib.mkd_dpmpp_step_ex(*args, P(kf), per + 1, P(xp), P(m0), n, None) == -1                        # n_per_sample does not divide n


@pytest.mark.parametrize('n,per', [(4 * 8 * 8 * 2, 256), (1003, 59), (4099, 4099)])
def test_ddim_step_kernel_with_factor_against_fp64(n, per):
    """test_ddim_step_matches_reference_formula's bound (rtol 2e-6, atol 1e-5) plus the one rounding of e = g * k (2^-24)"""
    lib = L()
    g = torch.Generator().manual_seed(n)
    B = n // per
    x, ec, eu, noise = (torch.randn(n, generator=g).to(DEV) for _ in range(4))
    a_t, a_prev, sigma, s = 0.0057755, 0.00728173, 0.05, 9.0
    s1m = float(np.sqrt(1 - a_t))
    kf = torch.empty(B, device=DEV)
    assert lib.mkd_cfg_rescale_factor(P(ec), P(eu), s, PHI, B, per, P(kf), None) == 0
    xp = torch.full((n,), float('nan'), device=DEV); x0 = torch.full((n,), float('nan'), device=DEV)
    assert lib.mkd_ddim_step_ex(P(x), P(ec), P(eu), s, a_t, a_prev, sigma, s1m, P(noise), 1.0, P(kf), per, P(xp), P(x0), n, None) == 0
    sync()
    xd, cd, ud, nd = (t.cpu().double() for t in (x, ec, eu, noise))
    e = (ud + s * (cd - ud)) * kf.cpu().double().repeat_interleave(per)
    r0 = (xd - s1m * e) / np.sqrt(a_t)
    rp = np.sqrt(a_prev) * r0 + np.sqrt(1 - a_prev - sigma ** 2) * e + sigma * nd
    rtol = 2e-6 + 2 ** -24
    assert torch.allclose(x0.cpu().double(), r0, rtol=rtol, atol=1e-5) and torch.allclose(xp.cpu().double(), rp, rtol=rtol, atol=1e-5)
    a1 = torch.empty_like(x); b1 = torch.empty_like(x); a2 = torch.empty_like(x); b2 = torch.empty_like(x)
    assert lib.mkd_ddim_step_ex(P(x), P(ec), P(eu), s, a_t, a_prev, sigma, s1m, P(noise), 1.0, None, 0, P(a1), P(b1), n, None) == 0
    assert lib.mkd_ddim_step(P(x), P(ec), P(eu), s, a_t, a_prev, sigma, s1m, P(noise), 1.0, P(a2), P(b2), n, None) == 0
    sync()
    assert torch.equal(a1, a2) and torch.equal(b1, b2) and not torch.equal(a1, xp)
    assert lib.mkd_ddim_step_ex(P(x), P(ec), None, s, a_t, a_prev, sigma, s1m, None, 1.0, P(kf), per, P(xp), P(x0), n, None) == -1


def _placed(vals, shift):
    """the values in a fresh device buffer, `shift` floats past its (at least 16-byte aligned) start"""
    buf = torch.empty(vals.numel() + 4, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:shift + vals.numel()]
    view.copy_(vals)
    return view


def _run_step(lib, solver, vals, coef, shift, guided, in_place, per, ddim_extras=False):
    """one stand-alone step of `solver` on operands placed at `shift`; returns the outputs (new latent, x0-prediction, xc) on the host"""
    n = vals['x'].numel()
    t = {k: _placed(v, shift) for k, v in vals.items()}
    nan = lambda: _placed(torch.full((n,), float('nan')), shift)
    x_out = t['x'] if in_place else nan()
    e_u, scale = (P(t['e_u']), 9.0) if guided else (None, 1.0)
    kf = None
    if guided:
        kf = torch.empty(n // per, device=DEV)
        assert lib.mkd_cfg_rescale_factor(P(t['e_c']), P(t['e_u']), scale, PHI, n // per, per, P(kf), None) == 0
    if solver == 'ddim':
        p0 = None if ddim_extras else nan()
        noise, sigma = (P(t['m1']), 0.05) if ddim_extras else (None, 0.0)
        a_t, a_prev = 0.0057755, 0.00728173
        head = (P(t['x']), P(t['e_c']), e_u, scale, a_t, a_prev, sigma, float(np.sqrt(1 - a_t)), noise, 0.8)
        rc = (lib.mkd_ddim_step_ex(*head, P(kf), per, P(x_out), P(p0), n, None) if guided else
              lib.mkd_ddim_step(*head, P(x_out), P(p0), n, None))
        outs = (x_out, p0)
    elif solver == 'dpm':
        p0 = nan()
        head = (P(t['x']), P(t['e_c']), e_u, scale, (C.c_float * 6)(*coef.tolist()), P(t['m1']), P(t['m2']))
        rc = (lib.mkd_dpmpp_step_ex(*head, P(kf), per, P(x_out), P(p0), n, None) if guided else
              lib.mkd_dpmpp_step(*head, P(x_out), P(p0), n, None))
        outs = (x_out, p0)
    else:
        p0 = nan()
        xc_out = t['xc'] if in_place else nan()
        head = (P(t['x']), P(t['xc']), P(t['e_c']), e_u, scale, (C.c_float * 12)(*coef.tolist()), P(t['m1']), P(t['m2']), P(t['m3']))
        rc = (lib.mkd_unipc_step_ex(*head, P(kf), per, P(x_out), P(xc_out), P(p0), n, None) if guided else
              lib.mkd_unipc_step(*head, P(x_out), P(xc_out), P(p0), n, None))
        outs = (x_out, p0, xc_out)
    assert rc == 0, lib.mkd_last_error()
    sync()
    return [None if o is None else o.cpu() for o in outs]


@pytest.mark.parametrize('solver', ['ddim', 'dpm', 'unipc'])
@pytest.mark.parametrize('n,per', [(512, 256), (1028, 257), (1003, 59)])      # 16-byte form twice (one past a multiple of 256 / 1024), scalar only
def test_step_kernel_forms_and_aliasing(solver, n, per):
    """One walker serves every solver: on 16-byte aligned operands (the 16-byte form where n % 4 == 0) and on the same values 4 bytes
    further (always the scalar form) a step gives the same bits, and in place (x_prev is x, xc_out is xc_prev) the bits of out of
    place.  Unguided, and guided with rescale factors; DDIM also with the eta term's noise and no pred_x0.  Every history plane is read
    (an order-3 entry from the middle of the table).  What the values must be is test_*_step_kernel*_against_fp64's business."""
    lib = L()
    _, a, ap = dref.grid(20)
    coef = None
    if solver == 'dpm':
        coef = dpmpp_table(a, ap, 3, True)[0][10]
        assert coef[4] != 0 and coef[5] != 0
    elif solver == 'unipc':
        coef = unipc_table(a, ap, 3, True, True)[0][10]
        assert all(coef[j] != 0 for j in (2, 4, 5, 6, 9, 10))
    g = torch.Generator().manual_seed(7 * n + len(solver))
    vals = {k: torch.randn(n, generator=g) for k in ('x', 'e_c', 'e_u', 'm1', 'm2', 'm3', 'xc')}
    variants = [dict(guided=False), dict(guided=True)] + ([dict(guided=True, ddim_extras=True)] if solver == 'ddim' else [])
    seen = []
    for v in variants:
        base = _run_step(lib, solver, vals, coef, 0, in_place=False, per=per, **v)
        assert all(o is None or torch.isfinite(o).all() for o in base) and not torch.equal(base[0], vals['x'])
        for shift, in_place in ((1, False), (0, True), (1, True)):
            got = _run_step(lib, solver, vals, coef, shift, in_place=in_place, per=per, **v)
            for name, b, o in zip(('x_out', 'p0', 'xc_out'), base, got):
                assert (b is None and o is None) or torch.equal(b, o), f'{solver} {v} shift {shift} in place {in_place}: {name} differs'
        seen.append(base[0])
    assert all(not torch.equal(seen[0], s) for s in seen[1:])          # guidance (and the noise) do change the result


# ---- 3. one arithmetic: graph replay == linear segments == eager, final latent and every trace row -----------------------------------
def loop_forms(I, S, sch50):
    """(name, method, cfg, per-call kwargs builder) of the loop forms under test on the first S entries of a 50-entry schedule"""
    ts = [int(t) for t in sch50.ddim_timesteps[:S]]
    a, ap, s1 = (v[:S] for v in (sch50.ddim_alphas, sch50.ddim_alphas_prev, sch50.ddim_sqrt_one_minus_alphas))
    g = torch.Generator().manual_seed(77)
    noise = torch.randn(S, 2, 4, 8, 8, generator=g).to(DEV)
    q_noise = torch.randn(S, 2, 4, 8, 8, generator=g).to(DEV)
    eta_sig = sampler.Schedule().make_ddim(50, 0.5).ddim_sigmas[:S]
    sa = sampler.Schedule().alphas_cumprod64
    masked = dict(x0=I['x0'], mask=I['mask'], q_sqrt_ac=[float(np.sqrt(sa[t])) for t in ts], q_sqrt_1m_ac=[float(np.sqrt(1 - sa[t])) for t in ts],
                  q_noise=q_noise)
    ddim = lambda eng, **k: eng.sample(I['x_T'], ts, a, ap, s1, **k)
    dpm = lambda eng, **k: eng.sample_dpmpp(I['x_T'], ts, a, ap, order=2, **k)
    return [('ddim', ddim, {}), ('ddim eta', ddim, dict(sigmas=eta_sig, noise=noise)), ('ddim masked', ddim, masked), ('dpm2', dpm, {})]


@pytest.mark.parametrize('S', [3, 7, 10])          # below graph_steps, one 5-step graph plus a tail, two graphs
def test_loop_forms_give_the_same_bits(engines, S):
    one, seg = engines
    I = inputs()
    sch50 = sampler.Schedule().make_ddim(50)
    for cfg in (1.0, 9.0):
        prepare(one, I, cfg); prepare(seg, I, cfg)
        for name, run, kw in loop_forms(I, S, sch50):
            for phi in ((0.0, PHI) if cfg != 1.0 else (0.0,)):
                base = run(one, cfg_scale=cfg, use_graph=True, guidance_rescale=phi, **kw)                   # untraced
                for Lt in (1, 3, 100):
                    outs = [run(one, cfg_scale=cfg, use_graph=True, log_every_t=Lt, want_trace=True, guidance_rescale=phi, **kw),
                            run(one, cfg_scale=cfg, use_graph=False, log_every_t=Lt, want_trace=True, guidance_rescale=phi, **kw),
                            run(seg, cfg_scale=cfg, use_graph=True, log_every_t=Lt, want_trace=True, guidance_rescale=phi, **kw)]
                    what = f'{name} S {S} L {Lt} cfg {cfg} phi {phi}'
                    rows = sample_log_rows(S, Lt)
                    for form, o in zip(('graph', 'eager', 'segments'), outs):
                        assert tuple(o[1].shape) == tuple(o[2].shape) == (rows, 2, 4, 8, 8), what
                        assert all(torch.isfinite(t).all() for t in o), f'{form}: non-finite ({what})'
                        for t, r in zip(o, outs[0]):
                            assert torch.equal(t, r), f'{form} != graph ({what})'
                    lat, xs, x0s = outs[0]
                    assert torch.equal(lat, base), f'the trace moved the latent ({what})'
                    assert torch.equal(xs[-1], lat) and not torch.equal(x0s[-1], lat)          # the last row is the last step's
                    if Lt == 1 and S > 1:
                        assert not torch.equal(xs[0], xs[1]) and not torch.equal(x0s[0], x0s[1])
            if cfg != 1.0:          # the rescale moves the latent, and phi is read per call (no re-capture needed for a new phi)
                p0 = run(one, cfg_scale=cfg, use_graph=True, **kw)
                p3 = run(one, cfg_scale=cfg, use_graph=True, guidance_rescale=0.3, **kw)
                p7 = run(one, cfg_scale=cfg, use_graph=True, guidance_rescale=PHI, **kw)
                assert metrics(p7, p0)[0] > 3e-2 and metrics(p3, p0)[0] > 1e-2 and metrics(p7, p3)[0] > 1e-2, name
                assert torch.equal(p3, run(one, cfg_scale=cfg, use_graph=False, guidance_rescale=0.3, **kw)), name


# ---- 4. ... == the per-step class loop (a callback forces it) ---------------------------------------------------------------------------
def sampler_runs(m, I, S, Lt, scale, phi):
    """{name: fn(callback) -> (latent, intermediates)} over the first S entries of the samplers' 50-entry schedule"""
    c = {'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]}
    uc = {'c_crossattn': [I['uctx']], 'c_concat': [I['hint']]} if scale != 1.0 else None
    out = {}
    for name, eta, masked in (('ddim', 0.0, False), ('ddim eta', 0.5, False), ('ddim masked', 0.0, True)):
        def run(callback, eta=eta, masked=masked):
            smp = DDIMSampler(m)
            smp.make_schedule(50, ddim_eta=eta, verbose=False)
            torch.manual_seed(90)
            return smp.ddim_sampling(c, (2, 4, 8, 8), x_T=I['x_T'], callback=callback, log_every_t=Lt, unconditional_guidance_scale=scale,
                                     unconditional_conditioning=uc, timesteps=smp.ddim_timesteps[:S], guidance_rescale=phi,
                                     **(dict(mask=I['mask'], x0=I['x0']) if masked else {}))
        out[name] = run

    def run_dpm(callback):
        smp = DPMSolverSampler(m)
        smp.make_schedule(50)
        inter = {'x_inter': [I['x_T']], 'pred_x0': [I['x_T']]}
        # (DPMSolverSampler.sample builds its own S-entry grid; the loop over the first S entries of a schedule is its _loop)
        img = smp._loop(I['x_T'], c, S, scale, uc, 2, True, callback, None, None, trace=(Lt, inter), phi=phi if uc is not None else 0.0)
        return img, inter
    out['dpm2'] = run_dpm
    return out


@pytest.mark.parametrize('S', [3, 7, 10])
def test_in_library_loop_equals_the_class_loop(mm, S):
    m, _ = mm
    I = inputs()
    for scale, phi in ((1.0, 0.0), (9.0, 0.0), (9.0, PHI)):
        for Lt in (1, 3, 100):
            for name, run in sampler_runs(m, I, S, Lt, scale, phi).items():
                what = f'{name} S {S} L {Lt} scale {scale} phi {phi}'
                lat, inter = run(None)
                lat_s, inter_s = run(lambda i: None)
                assert torch.equal(lat, lat_s), f'latent: {what}'
                for key in ('x_inter', 'pred_x0'):
                    assert len(inter[key]) == len(inter_s[key]) == 1 + sample_log_rows(S, Lt), f'{key}: {what}'
                    for j, (a_, b_) in enumerate(zip(inter[key], inter_s[key])):
                        assert torch.equal(a_, b_), f'{key}[{j}]: {what}'
                assert torch.equal(inter['x_inter'][-1], lat)
    # the eager in-library loop through the samplers as well
    m.sample_use_graph = False
    try:
        for name, run in sampler_runs(m, I, S, 3, 9.0, PHI).items():
            lat, inter = run(None)
            lat_s, inter_s = run(lambda i: None)
            assert torch.equal(lat, lat_s) and all(torch.equal(a_, b_) for a_, b_ in zip(inter['pred_x0'], inter_s['pred_x0'])), name
    finally:
        m.sample_use_graph = True


# ---- 5. shared state ---------------------------------------------------------------------------------------------------------------------
def test_plain_call_after_traced_and_rescaled_calls_keeps_its_bits(engines):
    one, seg = engines
    I = inputs()
    sch = sampler.Schedule().make_ddim(10)
    ts = [int(t) for t in sch.ddim_timesteps]
    for eng in (one, seg):
        for cfg in (1.0, 9.0):
            prepare(eng, I, cfg)
            ddim = lambda **k: eng.sample(I['x_T'], ts, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas, cfg_scale=cfg, **k)
            dpm = lambda **k: eng.sample_dpmpp(I['x_T'], ts, sch.ddim_alphas, sch.ddim_alphas_prev, order=2, cfg_scale=cfg, **k)
            for g in (True, False):
                before = (ddim(use_graph=g), dpm(use_graph=g))
                for run in (ddim, dpm):
                    run(use_graph=g, want_trace=True, log_every_t=2)
                    run(use_graph=g, want_trace=True, log_every_t=1, guidance_rescale=PHI)
                    run(use_graph=g, guidance_rescale=1.0)
                assert torch.equal(ddim(use_graph=g), before[0]) and torch.equal(dpm(use_graph=g), before[1]), f'cfg {cfg} graph {g}'
                eng.debug_poison()
                assert torch.equal(ddim(use_graph=g), before[0]) and torch.equal(dpm(use_graph=g), before[1]), f'poisoned: cfg {cfg} graph {g}'
                eng.debug_poison()
                t1 = ddim(use_graph=g, want_trace=True, log_every_t=3, guidance_rescale=PHI)
                t2 = ddim(use_graph=g, want_trace=True, log_every_t=3, guidance_rescale=PHI)
                assert all(torch.equal(a_, b_) for a_, b_ in zip(t1, t2))


def test_step_launch_count(engines):
    """the old forms' counts do not move (a traced step launches what an untraced one does); the rescaled guided step is one launch more"""
    one, _ = engines
    I = inputs()
    sch = sampler.Schedule().make_ddim(10)
    ts = [int(t) for t in sch.ddim_timesteps]
    prepare(one, I, 9.0)
    old = [one.step_launches(g, c) for g in (True, False) for c in (False, True)]
    raw = [one.lib.mkd_step_launches_ex(one._ctx, g, c) for g in (1, 0) for c in (0, 1)]
    assert old == raw and old[1] == old[0] + 1 and old[3] == old[2] + 1 and one.lib.mkd_step_launches(one._ctx) == old[0]
    one.sample(I['x_T'], ts, sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas, cfg_scale=9.0, use_graph=True,
               want_trace=True, log_every_t=1, guidance_rescale=PHI)
    one.sample_dpmpp(I['x_T'], ts, sch.ddim_alphas, sch.ddim_alphas_prev, cfg_scale=9.0, use_graph=False, want_trace=True, guidance_rescale=PHI)
    assert [one.step_launches(g, c) for g in (True, False) for c in (False, True)] == old
    for g in (True, False):
        assert one.step_launches(g, True, rescale=True) == one.step_launches(g, True) + 1
        assert one.step_launches(g, False, rescale=True) == one.step_launches(g, False)          # no guidance: not engaged
        assert one.lib.mkd_step_launches_ex(one._ctx, int(g), 2) == one.step_launches(g, True) + 1


def test_argument_checks(engines):
    one, _ = engines
    I = inputs()
    prepare(one, I, 9.0)
    S = 7
    sch = sampler.Schedule().make_ddim(50)
    ts = (C.c_int64 * S)(*[int(t) for t in sch.ddim_timesteps[:S]])
    a, ap, s1 = ((C.c_float * S)(*[float(v) for v in t[:S]]) for t in (sch.ddim_alphas, sch.ddim_alphas_prev, sch.ddim_sqrt_one_minus_alphas))
    out = torch.empty_like(I['x_T'])
    rows = sample_log_rows(S, 3)
    assert rows == one.lib.mkd_sample_log_rows(S, 3) == 3 and one.lib.mkd_sample_log_rows(S, 0) == -1 and one.lib.mkd_sample_log_rows(0, 1) == -1
    buf = torch.empty(rows + 1, *I['x_T'].shape, device=DEV)

    def call(dpm, ex, graph=1):
        if dpm:
            return one.lib.mkd_sample_dpmpp_ex(one._ctx, P(I['x_T']), 2, S, ts, a, ap, 2, 1, None, ex, 9.0, P(out), graph, None)
        return one.lib.mkd_sample_masked_ex(one._ctx, P(I['x_T']), 2, S, ts, a, ap, s1, None, None, 1.0, None, ex, 9.0, P(out), graph, None)
    E = mlib.SampleExtrasC
    for dpm in (False, True):
        for graph in (1, 0):
            for bad in (E(3, rows + 1, buf.data_ptr(), buf.data_ptr(), 0.0), E(3, rows - 1, buf.data_ptr(), None, 0.0),
                        E(0, rows, None, buf.data_ptr(), 0.0), E(3, 0, buf.data_ptr(), buf.data_ptr(), 0.0),
                        E(3, rows, None, None, 1.5), E(3, rows, None, None, -0.25), E(3, rows, None, None, float('nan'))):
                assert call(dpm, C.byref(bad), graph) == -1, (dpm, graph, bad.log_every_t, bad.rows, bad.guidance_rescale)
        # one list alone, and a struct that asks for nothing (rows then unused): fine; ex == NULL is the old entry
        x0_only = E(3, rows, None, buf.data_ptr(), 0.0)
        assert call(dpm, C.byref(x0_only)) == 0 and call(dpm, C.byref(E(0, 0, None, None, 0.0))) == 0
        sync()
        plain = out.clone()
        assert call(dpm, None) == 0
        sync()
        assert torch.equal(out, plain)
    with pytest.raises(ValueError):
        one.sample(I['x_T'], [1], [0.9], [0.99], [0.3], cfg_scale=9.0, guidance_rescale=1.2)
    with pytest.raises(ValueError):
        one.sample(I['x_T'], [1], [0.9], [0.99], [0.3], cfg_scale=9.0, want_trace=True, log_every_t=0)


# ---- 6. trajectory against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['ddim', 'dpm2'])
def test_rescaled_trajectory_vs_oracle(mm, which):
    """10 steps, guidance 9, phi 0.7 against the restated loop over the fp32 oracle nets.  Precondition (CPU side): the restated
    rescaled latent lies >= 3 x the limit away from the restated un-rescaled one, so a missing or wrong rescale cannot pass.
    Measured on the MI355X (MEASURED_RESCALED): DDIM rel-L2 1.67e-2 / cos 0.99986, DPM-Solver++ order 2 1.55e-2 / 0.99988; the restated
    rescaled latent lies 0.256 / 0.243 from the un-rescaled one; the per-step factors run from 0.55 to 0.95."""
    m, sd = mm
    I = inputs()
    c = {'c_crossattn': [I['ctx']], 'c_concat': [I['hint']]}
    uc = {'c_crossattn': [I['uctx']], 'c_concat': [I['hint']]}
    cpu = lambda d: {k: [t.cpu() for t in v] for k, v in d.items()}
    eps_fn = sampler.make_eps_fn(sd, OCFG)
    sch = sampler.Schedule().make_ddim(10)
    factors = []
    if which == 'ddim':
        ref, _, x0s = xref.ddim_loop(eps_fn, sch, I['x_T'].cpu(), cpu(c), 9.0, cpu(uc), PHI, 1, factors=factors)
        plain, _, _ = xref.ddim_loop(eps_fn, sch, I['x_T'].cpu(), cpu(c), 9.0, cpu(uc), 0.0, 1)
        out, inter = DDIMSampler(m).sample(10, 2, (4, 8, 8), conditioning=c, x_T=I['x_T'], eta=0.0, verbose=False, log_every_t=1,
                                           unconditional_guidance_scale=9.0, unconditional_conditioning=uc, guidance_rescale=PHI)
    else:
        args = (sch.ddim_timesteps, sch.ddim_alphas.numpy(), sch.ddim_alphas_prev.numpy(), I['x_T'].cpu(), cpu(c), 2, True, 9.0, cpu(uc))
        ref, _, x0s = xref.dpm_loop(eps_fn, *args, PHI, 1, factors=factors)
        plain, _, _ = xref.dpm_loop(eps_fn, *args, 0.0, 1)
        out, inter = DPMSolverSampler(m).sample(10, 2, (4, 8, 8), conditioning=c, x_T=I['x_T'], order=2, log_every_t=1,
                                                unconditional_guidance_scale=9.0, unconditional_conditioning=uc, guidance_rescale=PHI)
    ks = torch.stack(factors)
    moved = metrics(ref, plain)[0]
    r, cs = metrics(out, ref)
    r0, _ = metrics(inter['pred_x0'][-1], x0s[-1])
    print(f'[parity] rescaled {which}, 10-step latent vs oracle: rel-L2 {r:.4e} cos {cs:.6f}; last pred_x0 rel-L2 {r0:.4e}; '
          f'restated rescaled vs plain {moved:.4f}; factors {ks.min().item():.3f} .. {ks.max().item():.3f}')
    assert MEASURED_RESCALED[which] is not None, 'no measured distance recorded'
    lim = 3.0 * MEASURED_RESCALED[which]
    assert moved >= 3.0 * lim, f'precondition: restated rescaled vs un-rescaled {moved:.4f} < 3 x limit {lim:.4f}'
    assert (ks[:, 0] - ks[:, 1]).abs().max() > 1e-2                 # the two samples' factors differ
    assert cs >= COS_CAP and r <= lim, f'rel-L2 {r:.4e} > {lim:.4e} or cos {cs:.6f}'


# ---- 7. the model surface -------------------------------------------------------------------------------------------------------------------
def test_log_results_denoise_rows(mm):
    m, _ = mm
    g = torch.Generator().manual_seed(70)
    B = 2
    batch = {'src_img': torch.rand(B, 3, 64, 64, generator=g), 'ref_img': torch.rand(B, 3, 64, 64, generator=g),
             'txt_emb': torch.randn(B, 77, 64, generator=g)}
    x_T = torch.randn(B, 4, 8, 8, generator=g).to(DEV)
    base = m.log_results(batch, 0, x_T=x_T)
    m.denoise_rows, m.log_every_t, m.guidance_rescale = True, 2, PHI
    try:
        log = m.log_results(batch, 0, x_T=x_T)
    finally:
        m.denoise_rows, m.log_every_t, m.guidance_rescale = False, 100, 0.0
    assert set(log) == set(base) | {'denoise_row', 'denoise_row_latent', 'denoise_row_cfg_scale_9.00', 'denoise_row_cfg_scale_9.00_latent'}
    assert torch.equal(log['samples_latent'], base['samples_latent']) and torch.equal(log['samples'], base['samples'])
    assert metrics(log['samples_cfg_scale_9.00_latent'], base['samples_cfg_scale_9.00_latent'])[0] > 1e-2       # the guided pass is rescaled
    n = 1 + sample_log_rows(m.ddim_steps, 2)                             # list entries: x_T, then the logged steps
    for key, final in (('denoise_row', 'samples_latent'), ('denoise_row_cfg_scale_9.00', 'samples_cfg_scale_9.00_latent')):
        lat, img = log[key + '_latent'], log[key]
        assert tuple(lat.shape) == (B * n, 4, 8, 8) and tuple(img.shape) == (B * n, 3, 64, 64) and torch.isfinite(img).all()
        for j in range(n):                                               # one image per list entry per sample, 'b n' order
            col = torch.stack([lat[b * n + j] for b in range(B)])
            dec = m.decode_first_stage(col)
            for b in range(B):
                assert torch.equal(img[b * n + j], dec[b]), f'{key}: sample {b} entry {j}'
        assert torch.equal(torch.stack([lat[b * n] for b in range(B)]), x_T)
        assert not torch.equal(lat[n - 1], lat[n - 2])
    # the rows are the sampler's pred_x0 list of the same call
    c = {'c_concat': [torch.cat((batch['src_img'], batch['ref_img']), 1).to(DEV)], 'c_crossattn': [batch['txt_emb'].to(DEV)]}
    _, inter = DDIMSampler(m).sample(m.ddim_steps, B, (4, 8, 8), conditioning=c, x_T=x_T, eta=0.0, verbose=False, log_every_t=2)
    assert len(inter['pred_x0']) == n
    for j in range(n):
        assert torch.equal(inter['pred_x0'][j], torch.stack([log['denoise_row_latent'][b * n + j] for b in range(B)]))
    again = m.log_results(batch, 0, x_T=x_T)
    assert set(again) == set(base) and all(torch.equal(again[k], base[k]) for k in base)           # the default path is untouched


def test_runs_test_py_writes_the_denoise_grids(tmp_path):
    from PIL import Image
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--pairs', '2', '--batch-size', '2', '--res', '64',
                        '--ddim-steps', '4', '--seed', '5', '--denoise-rows', '--log-every-t', '2', '--guidance-rescale', '0.7',
                        '--out', str(out)], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    root = out / 'makeupdiffuse_mi355x'
    names = sorted(os.listdir(root))
    assert names == ['control_ref_0000.png', 'control_src_0000.png', 'denoise_row_0000.png', 'denoise_row_cfg_scale_9.00_0000.png',
                     'samples_0000.png', 'samples_cfg_scale_9.00_0000.png'], names
    for nm in ('denoise_row_0000.png', 'denoise_row_cfg_scale_9.00_0000.png'):
        assert np.asarray(Image.open(root / nm)).std() > 1.0
    lat = torch.load(out / 'latents_0000.pt')
    n = 1 + sample_log_rows(4, 2)
    assert tuple(lat['denoise_row_latent'].shape) == (2 * n, 4, 8, 8) and tuple(lat['denoise_row'].shape) == (2 * n, 3, 64, 64)
    assert torch.isfinite(lat['denoise_row_cfg_scale_9.00']).all()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'runs', 'test.py'), '--guidance-rescale', '1.5'], capture_output=True, text=True,
                       timeout=900, cwd=str(tmp_path))
    assert r.returncode != 0 and '--guidance-rescale' in r.stderr
