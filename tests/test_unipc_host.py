"""CPU: the UniPC predictor-corrector sampler.  The float64 restatement (tests/unipc_ref.py) against DPM-Solver++ with the corrector
off, polynomial exactness of the solved updates, the twelve-number rows as the two linear forms, the Gaussian toy against
DPM-Solver++ 2M, the library's host-only table against the Python coefficients, every refusal that needs no device, and
UniPCSampler's plumbing on host stand-in models."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dpm_solver_ref as dref
import unipc_ref as uref
from makeupdiffuse_amd import lib as mlib
from makeupdiffuse_amd.diffmk.makeup_diffuse import TestDiffuseModel
from makeupdiffuse_amd.dpm_solver import DPMSolverSampler, dpmpp_coefficients
from makeupdiffuse_amd.engine import dpmpp_table, sample_log_rows, unipc_table
from makeupdiffuse_amd.unipc import UniPCSampler, unipc_coefficients
from oracle import sampler
from test_dpm_solver_host import HostModel

S_ALL = (5, 9, 10, 20, 50)


def dpm_rows_run(m_fn, alphas, alphas_prev, x, order, lof=True):
    """a trajectory driven by dpmpp_coefficients: x <- c_x x + c_0 m_k + c_1 m_{k-1} + c_2 m_{k-2}"""
    coef, _ = dpmpp_coefficients(alphas, alphas_prev, order, lof)
    n = len(alphas)
    hist = [None, None]
    for k in range(n):
        c = coef[n - 1 - k]
        m0 = m_fn(k, x)
        x = c[2] * x + c[3] * m0
        if c[4] != 0.0:
            x = x + c[4] * hist[0]
        if c[5] != 0.0:
            x = x + c[5] * hist[1]
        hist = [m0, hist[0]]
    return x


def wavy_model(a_grid):
    """an x-dependent, step-dependent x0-prediction on vectors (a stand-in: any smooth map will do)"""
    return lambda k, x: np.tanh(0.7 * x + 0.1 * k) * (1.0 + 0.3 * math.sqrt(a_grid[k])) + 0.05 * x


# ---- 1. the corrector off: DPM-Solver++ ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', S_ALL)
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('lof', [True, False])
def test_without_corrector_orders_one_and_two_are_dpm_solver_pp(S, order, lof):
    """the restatement with the corrector off against a dpmpp_coefficients-driven trajectory: <= 1e-12 (order 1: the DDIM map; order 2:
    the q = 1 predictor shortcut is the 2M step)"""
    _, a, ap = dref.grid(S)
    m_fn = wavy_model(uref.grid_points(a, ap))
    x_T = np.random.default_rng(1).standard_normal(64)
    uni = uref.run(m_fn, a, ap, x_T, order, lof, corrector=False)
    dpm = dpm_rows_run(m_fn, a, ap, x_T, order, lof)
    d = np.abs(uni - dpm).max()
    print(f'[unipc] corrector off vs DPM-Solver++ rows, S {S} order {order} lof {lof}: max |delta| {d:.3e}')
    assert d <= 1e-12
    with_cor = uref.run(m_fn, a, ap, x_T, order, lof, corrector=True)
    assert np.abs(with_cor - dpm).max() > 1e-6                   # (the corrector is another map: not a vacuous equality)


# ---- 2. polynomial exactness ------------------------------------------------------------------------------------------------------
def exact_integral(poly, h):
    """int_0^h e^(u-h) poly(u) du by Gauss-Legendre quadrature (48 nodes: exact to rounding for these smooth integrands)"""
    t, w = np.polynomial.legendre.leggauss(48)
    u = 0.5 * h * (t + 1.0)
    return float(np.sum(0.5 * h * w * np.exp(u - h) * poly(u)))


@pytest.mark.parametrize('S', [10, 20, 50])
def test_solved_updates_integrate_polynomials_exactly(S):
    """An x-independent m(lambda), a polynomial of degree q, through one update with q nodes: the analytic
    (sigma_t / sigma_s) x_s + alpha_t int_0^h e^(u-h) m(lambda_s + u) du to 1e-12, for the predictor with q = 2 and q = 3 nodes and the
    corrector with q = 2 and q = 3 (whose last node is the new point) - in the restatement, and in the library's rows wherever they hold
    a solved update (order 3: the predictor of steps k >= 2 has q = 2, the corrector of step 2 q = 2, of steps k >= 3 q = 3)."""
    _, a, ap = dref.grid(S)
    pts = uref.grid_points(a, ap)
    lams = [uref.lam(v) for v in pts]
    rng = np.random.default_rng(2)
    x_s = float(rng.standard_normal())
    worst = 0.0
    for k in (3, S // 2, S - 1):
        for kind, q in (('predictor', 2), ('predictor', 3), ('corrector', 2), ('corrector', 3)):
            cs = rng.standard_normal(q + 1)
            base, target = (k, k + 1) if kind == 'predictor' else (k - 1, k)
            poly = lambda u: sum(c * u ** i for i, c in enumerate(cs))
            m_at = lambda j: poly(lams[j] - lams[base])
            if kind == 'predictor':
                nodes = [(lams[base - j], m_at(base - j)) for j in range(1, q + 1)]
            else:
                nodes = [(lams[base - j], m_at(base - j)) for j in range(1, q)] + [(lams[target], m_at(target))]
            out = uref.update(x_s, m_at(base), pts[base], pts[target], nodes, kind)
            h = lams[target] - lams[base]
            want = math.sqrt(1.0 - pts[target]) / math.sqrt(1.0 - pts[base]) * x_s + math.sqrt(pts[target]) * exact_integral(poly, h)
            worst = max(worst, abs(out - want))
            assert abs(out - want) <= 1e-12 * max(1.0, abs(want)), (kind, q, k, out, want)
    coef, orders = unipc_coefficients(a, ap, 3, True, True)
    for k in range(2, S):
        c = coef[S - 1 - k]
        # predictor of step k: two nodes, degree 2
        cs = rng.standard_normal(3)
        poly = lambda u: sum(cc * u ** i for i, cc in enumerate(cs))
        m = [poly(lams[k - j] - lams[k]) for j in range(3)]
        out = c[7] * x_s + c[8] * m[0] + c[9] * m[1] + c[10] * m[2]
        want = math.sqrt(1.0 - pts[k + 1]) / math.sqrt(1.0 - pts[k]) * x_s + math.sqrt(pts[k + 1]) * exact_integral(poly, lams[k + 1] - lams[k])
        if orders[S - 1 - k] == 3:
            worst = max(worst, abs(out - want))
            assert abs(out - want) <= 1e-12 * max(1.0, abs(want)), ('row predictor', k)
        # corrector of step k: q = p_{k-1} nodes, degree q, base k - 1
        q = int(orders[S - k])
        cs = rng.standard_normal(q + 1)
        poly = lambda u: sum(cc * u ** i for i, cc in enumerate(cs))
        m = [poly(lams[k - j] - lams[k - 1]) for j in range(min(4, k + 1))] + [0.0] * 4
        out = c[2] * x_s + c[3] * m[0] + c[4] * m[1] + c[5] * m[2] + c[6] * m[3]
        want = math.sqrt(1.0 - pts[k]) / math.sqrt(1.0 - pts[k - 1]) * x_s + math.sqrt(pts[k]) * exact_integral(poly, lams[k] - lams[k - 1])
        assert q in (2, 3)
        worst = max(worst, abs(out - want))
        assert abs(out - want) <= 1e-12 * max(1.0, abs(want)), ('row corrector', k, q)
    print(f'[unipc] polynomial exactness, S {S}: worst |delta| {worst:.3e}')


@pytest.mark.parametrize('S', S_ALL)
@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('corrector', [True, False])
def test_constant_x0_prediction_is_integrated_exactly(S, order, corrector):
    """degree 0: every update, shortcut or solved, carries a constant m exactly, so the whole trajectory is the ODE solution"""
    g = torch.Generator().manual_seed(5)
    cst = torch.randn(1, 4, 3, 3, generator=g, dtype=torch.float64)
    x_T = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64)
    alpha_of = lambda t: sampler.Schedule().alphas_cumprod.double()[t].view(-1, 1, 1, 1)

    def eps(x, t, c):
        a = alpha_of(t)
        return (x - a.sqrt() * cst) / (1.0 - a).sqrt()
    ts, a, ap = dref.grid(S)
    a_T, a_0 = float(a[-1]), float(ap[0])
    exact = math.sqrt(a_0) * cst + math.sqrt((1.0 - a_0) / (1.0 - a_T)) * (x_T - math.sqrt(a_T) * cst)
    ref = uref.unipc(eps, ts, a, ap, x_T, order=order, corrector=corrector)
    assert (ref - exact).abs().max().item() <= 1e-12, 'restatement'
    if 1000 % S:
        return                                               # (S = 9: make_schedule's uniform grid has no 9-entry form)
    for lof in (True, False):
        out, _ = UniPCSampler(HostModel(eps)).sample(S, 2, (4, 3, 3), x_T=x_T, order=order, lower_order_final=lof, corrector=corrector)
        d = (out - exact).abs().max().item()
        assert d <= 1e-12, f'S {S} order {order} corrector {corrector}: {d:.3e}'


# ---- 3. the rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', S_ALL)
@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('corrector', [True, False])
def test_rows_reproduce_the_restatement(S, order, corrector):
    """unipc_coefficients' rows, driven as the two linear forms, against the restatement's loop (every x~_{k+1}, x^c_k and m_k), and
    against the rows the restatement gives by linearity; the sampler's host loop runs the same rows"""
    _, a, ap = dref.grid(S)
    m_fn = wavy_model(uref.grid_points(a, ap))
    x_T = np.random.default_rng(3).standard_normal(64)
    for lof in (True, False):
        coef, orders = unipc_coefficients(a, ap, order, lof, corrector)
        t_ref, t_rows = [], []
        uref.run(m_fn, a, ap, x_T, order, lof, corrector, trace=t_ref)
        uref.run_rows(m_fn, coef, x_T, trace=t_rows)
        for k, (u, v) in enumerate(zip(t_ref, t_rows)):
            for name, p, q in zip(('x_next', 'xc', 'm'), u, v):
                assert np.abs(p - q).max() <= 1e-12, f'{name} of step {k}: {np.abs(p - q).max():.3e}'
        ref, ref_orders = uref.coefficients(a, ap, order, lof, corrector)
        assert coef.shape == (S, 12) and orders.tolist() == ref_orders.tolist() == dref.step_orders(S, order, lof)[::-1]
        assert ((coef == 0) == (ref == 0)).all() and np.allclose(coef, ref, rtol=1e-11, atol=0)
        assert (coef[:, 11] == 0).all()
        for i in range(S):
            k = S - 1 - i
            p_k, p_prev = orders[i], (orders[i + 1] if k >= 1 else 0)
            on = corrector and k >= 1
            assert (coef[i, 2] != 0) == on and (coef[i, 3] != 0) == on and (coef[i, 4] != 0) == on
            assert (coef[i, 5] != 0) == (on and p_prev >= 2) and (coef[i, 6] != 0) == (on and p_prev >= 3)
            assert (coef[i, 9] != 0) == (p_k >= 2) and (coef[i, 10] != 0) == (p_k >= 3)


# ---- 4. the Gaussian toy ------------------------------------------------------------------------------------------------------------
def test_order_two_with_corrector_beats_dpm_solver_2m_on_the_gaussian_toy():
    """64-dimensional Gaussian data (per-dimension variances 0.05 .. 4, seed 0), analytic eps, exact ODE solution, the yaml's
    scaled-linear schedule, uniform grid.  Relative error of the final latent, UniPC order 2 with the corrector / DPM-Solver++ 2M:
        10 evaluations   4.877e-2 / 5.954e-2
        20 evaluations   1.810e-2 / 2.520e-2
        50 evaluations   4.593e-3 / 7.290e-3
    (strictly smaller at each of them, which is what is asserted.  Not asserted, as measured: at 5 evaluations UniPC does not win,
    1.236e-1 / 1.127e-1; order 3 with the corrector is not better than order 2 at 10 evaluations on this toy, 8.660e-2.)"""
    toy = uref.GaussianToy(64, seed=0)
    uni = lambda m, a, ap, x: uref.run(m, a, ap, x, 2, True, True)
    rows = lambda m, a, ap, x: uref.run_rows(m, unipc_coefficients(a, ap, 2, True, True)[0], x)
    dpm = lambda m, a, ap, x: dpm_rows_run(m, a, ap, x, 2)
    for S in (10, 20, 50):
        e_uni, e_rows, e_dpm = toy.errors(S, uni), toy.errors(S, rows), toy.errors(S, dpm)
        print(f'[unipc] Gaussian toy, {S} evaluations: UniPC order 2 + corrector {e_uni:.4e} (rows {e_rows:.4e}), DPM-Solver++ 2M {e_dpm:.4e}')
        assert e_uni < e_dpm and e_rows < e_dpm
        assert abs(e_rows - e_uni) <= 1e-10
    assert toy.errors(50, uni) < toy.errors(20, uni) < toy.errors(10, uni)


# ---- 5. the library's table ---------------------------------------------------------------------------------------------------------
# max over the non-zero entries of |float table - float64 coefficients| / |float64 coefficients|, mkd_dpmpp_table against
# dpmpp_coefficients over orders 1 .. 3 on the S-entry uniform grid, measured on the CPU (one float rounding of a double: <= 2^-24 = 5.96e-8)
DPM_TABLE_DISTANCE = {10: 5.319e-8, 50: 5.762e-8}


def table_distance(tab, ref):
    nz = ref != 0
    assert ((tab != 0) == nz).all()
    return float(np.max(np.abs(tab.astype(np.float64)[nz] - ref[nz]) / np.abs(ref[nz])))


@pytest.mark.parametrize('S', [10, 50])
def test_table_against_the_python_coefficients(S):
    """mkd_unipc_table against unipc_coefficients: within 3 x the distance of mkd_dpmpp_table from dpmpp_coefficients on the same grid
    (DPM_TABLE_DISTANCE, re-measured here)"""
    _, a, ap = dref.grid(S)
    d_dpm = max(table_distance(dpmpp_table(a, ap, o, True)[0], dpmpp_coefficients(a, ap, o, True)[0]) for o in (1, 2, 3))
    print(f'[unipc] S {S}: mkd_dpmpp_table vs dpmpp_coefficients {d_dpm:.4e}')
    assert d_dpm <= DPM_TABLE_DISTANCE[S] * 1.001
    for order in (1, 2, 3):
        for lof in (True, False):
            for cor in (True, False):
                tab, so = unipc_table(a, ap, order, lof, cor)
                py, po = unipc_coefficients(a, ap, order, lof, cor)
                assert tab.dtype == np.float32 and tab.shape == (S, 12) and so.tolist() == po.tolist()
                d = table_distance(tab, py)
                print(f'[unipc] S {S} order {order} lof {lof} corrector {cor}: mkd_unipc_table vs unipc_coefficients {d:.4e}')
                assert d <= 3.0 * DPM_TABLE_DISTANCE[S]


def test_predictor_rows_are_the_dpmpp_rows_as_floats():
    """order 2 with the corrector off on the 10-entry grid: the five numbers a DPM-Solver++ order-2 row shares with a UniPC row are
    the same floats (why the two device loops give the same bits there)"""
    ts, a, ap, _ = (lambda s: ([int(t) for t in s.ddim_timesteps], s.ddim_alphas, s.ddim_alphas_prev, None))(sampler.Schedule().make_ddim(10))
    uni, _ = unipc_table(a, ap, 2, True, False)
    dpm, _ = dpmpp_table(a, ap, 2, True)
    assert np.array_equal(uni[:, [0, 1, 7, 8, 9]], dpm[:, [0, 1, 2, 3, 4]])


def test_refusals_need_no_device():
    lib = mlib.load()
    _, a, ap = dref.grid(10)
    n = len(a)
    out = (ctypes.c_float * (12 * n))()
    fa = lambda v: (ctypes.c_float * len(v))(*[float(x) for x in v])
    assert lib.mkd_unipc_table(n, fa(a), fa(ap), 2, 1, 1, out, None) == 0                   # step_order may be NULL
    for order in (0, 4, -1):
        assert lib.mkd_unipc_table(n, fa(a), fa(ap), order, 1, 1, out, None) == -1          # MKD_ERR_ARG
        with pytest.raises(ValueError):
            unipc_coefficients(a, ap, order)
        with pytest.raises(ValueError):
            unipc_table(a, ap, order)
    gap = list(ap); gap[4] = 0.5 * (ap[4] + ap[3])                                          # not contiguous: alphas_prev[4] != alphas[3]
    assert lib.mkd_unipc_table(n, fa(a), fa(gap), 2, 1, 1, out, None) == -1
    assert b'contiguous' in lib.mkd_last_error()
    with pytest.raises(ValueError, match='contiguous'):
        unipc_coefficients(a, gap)
    with pytest.raises(ValueError, match='contiguous'):
        unipc_table(a, gap)
    with pytest.raises(ValueError, match='contiguous'):
        uref.grid_points(a, gap)
    for bad_a, bad_p in ((list(a[:-1]) + [0.0], ap), (list(a[:-1]) + [1.0], ap), (a, [1.0] + list(ap[1:])), (a, [0.0] + list(ap[1:]))):
        assert lib.mkd_unipc_table(n, fa(bad_a), fa(bad_p), 2, 1, 1, out, None) == -1      # an alpha outside (0, 1)
        with pytest.raises(ValueError):
            unipc_coefficients(bad_a, bad_p)
    assert lib.mkd_unipc_table(n, fa(a[::-1]), fa(ap[::-1]), 2, 1, 1, out, None) == -1      # (neither contiguous nor increasing)
    rev_a = a[::-1]; rev_p = np.asarray([a[0] * 0.5] + list(rev_a[:-1]), dtype=np.float32)  # contiguous, but lambda decreases
    assert lib.mkd_unipc_table(n, fa(rev_a), fa(rev_p), 2, 1, 1, out, None) == -1
    assert b'lambda' in lib.mkd_last_error()
    with pytest.raises(ValueError, match='lambda'):
        unipc_coefficients(rev_a, rev_p)
    assert lib.mkd_unipc_table(0, fa(a), fa(ap), 2, 1, 1, out, None) == -1
    assert lib.mkd_unipc_table(n, None, fa(ap), 2, 1, 1, out, None) == -1
    assert lib.mkd_unipc_table(n, fa(a), None, 2, 1, 1, out, None) == -1
    assert lib.mkd_unipc_table(n, fa(a), fa(ap), 2, 1, 1, None, None) == -1
    # the step and the loop: null pointers are refused before any device call (no device here)
    row = (ctypes.c_float * 12)(*unipc_table(a, ap, 3)[0][0].tolist())
    one = ctypes.c_void_p(64)          # (never dereferenced: every call below is refused on its arguments)
    assert lib.mkd_unipc_step(None, one, one, None, 1.0, row, one, one, one, one, one, one, 16, None) == -1
    assert lib.mkd_unipc_step(one, one, one, None, 1.0, None, one, one, one, one, one, one, 16, None) == -1
    assert lib.mkd_unipc_step(one, one, one, None, 1.0, row, one, one, one, one, one, one, 0, None) == -1
    for hole in (1, 6, 7, 8):          # a non-zero a_c / q_j / p_j with a null x^c_{k-1} / m1 / m2 / m3
        args = [one, one, one, None, 1.0, row, one, one, one, one, one, one, 16, None]
        args[hole] = None
        assert lib.mkd_unipc_step(*args) == -1
        assert b'non-zero' in lib.mkd_last_error()
    assert lib.mkd_unipc_step_ex(one, one, one, None, 9.0, row, one, one, one, one, 8, one, one, one, 16, None) == -1      # k without eps_u
    assert lib.mkd_sample_unipc(None, one, 2, n, None, fa(a), fa(ap), 2, 1, 1, None, 1.0, one, 0, None) == -1               # null ctx
    assert lib.mkd_sample_unipc_ex(None, one, 2, n, None, fa(a), fa(ap), 2, 1, 1, None, None, 1.0, one, 0, None) == -1
    # the per-sample loop keeps its two solvers, and its refusal text
    rows = (mlib.SampleRowC * 1)()
    assert lib.mkd_step_table(rows, 1, 2, None, None, None, None) == -1
    assert lib.mkd_last_error() == b'mkd_sample_rows: solver must be 0 (DDIM) or 1 (DPM-Solver++)'


# ---- 6. the Python layer ---------------------------------------------------------------------------------------------------------------
def test_rejected_options():
    m = HostModel(lambda x, t, c: 0.1 * x)
    s = UniPCSampler(m)
    x_T = torch.randn(2, 4, 3, 3)
    for kw in (dict(eta=0.5), dict(score_corrector=object()), dict(dynamic_threshold=0.9), dict(corrector_kwargs={'a': 1}),
               dict(ucg_schedule=[1.0]), dict(quantize_x0=True), dict(temperature=0.5), dict(noise_dropout=0.1),
               dict(img_callback=print)):
        with pytest.raises(NotImplementedError):
            s.sample(4, 2, (4, 3, 3), x_T=x_T, **kw)
        with pytest.raises(NotImplementedError):
            DPMSolverSampler(m).sample(4, 2, (4, 3, 3), x_T=x_T, **kw)          # (the same options DPMSolverSampler rejects)
    s.sample(4, 2, (4, 3, 3), x_T=x_T, eta=0.0, verbose=False)                  # the call shape log_results uses
    for order in (0, 4):
        with pytest.raises(ValueError):
            s.sample(4, 2, (4, 3, 3), x_T=x_T, order=order)
    with pytest.raises(ValueError):
        s.sample(4, 2, (4, 3, 3), x_T=x_T, guidance_rescale=1.5)
    with pytest.raises(ValueError):
        s.sample(4, 2, (4, 3, 3), x_T=x_T, log_every_t=0)
    calls = len(m.calls)
    for kw in (dict(mask=torch.ones(2, 1, 3, 3), x0=torch.zeros(2, 4, 3, 3)), dict(mask=torch.ones(2, 1, 3, 3)), dict(x0=torch.zeros(2, 4, 3, 3))):
        with pytest.raises(NotImplementedError, match='masked'):
            s.sample(4, 2, (4, 3, 3), x_T=x_T, **kw)
    with pytest.raises(NotImplementedError, match='per-sample'):
        s.sample_specs([], (4, 3, 3), None)
    assert len(m.calls) == calls                                                # (nothing was evaluated)


def test_model_accepts_the_sampler_name():
    small = dict(in_channels=4, model_channels=64, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=2, num_heads=2,
                 context_dim=64, use_spatial_transformer=True, transformer_depth=1, legacy=False)
    mk = lambda **kw: TestDiffuseModel(control_stage_config={'params': dict(small, hint_channels=6, hint_widths=[16, 16, 32, 32, 32, 32, 64])},
                                       unet_config={'params': dict(small, out_channels=4)}, **kw)
    m = mk(sampler='unipc', solver_order=3, unipc_corrector=False)
    assert (m.sampler, m.solver_order, m.unipc_corrector) == ('unipc', 3, False)
    assert mk(sampler='unipc').unipc_corrector is True and mk().unipc_corrector is True
    with pytest.raises(ValueError, match="sampler must be 'ddim' or 'dpmpp'"):           # (the refusal text stays as it was)
        mk(sampler='euler')
    with pytest.raises(ValueError):
        mk(sampler='unipc', solver_order=4)
    # fix_background samples with a mask: refused before the batch is even looked at
    m = mk(sampler='unipc', fix_background=True)
    with pytest.raises(NotImplementedError, match='masked'):
        m.log_results({}, 0)
    with pytest.raises(NotImplementedError, match='masked'):
        m.transfer_photos([], [])
    with pytest.raises(NotImplementedError, match='per-sample'):
        mk(sampler='unipc').transfer_specs({'src_img': torch.rand(1, 3, 64, 64), 'ref_img': torch.rand(1, 3, 64, 64),
                                            'txt_emb': torch.randn(1, 77, 64)}, [])


# ---- 7. plumbing on a stand-in model ------------------------------------------------------------------------------------------------------
def test_unconditional_first_batching_callback_count_and_trace_lengths():
    m = HostModel(lambda x, t, c: 0.1 * x + c['v'])
    S, B = 5, 2
    x_T = torch.randn(B, 4, 3, 3)
    c = {'v': torch.full((B, 1, 1, 1), 2.0)}
    uc = {'v': torch.full((B, 1, 1, 1), -1.0)}
    seen = []
    out, inter = UniPCSampler(m).sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, unconditional_guidance_scale=3.0,
                                        unconditional_conditioning=uc, callback=seen.append)
    assert seen == list(range(S))
    assert len(m.calls) == S and all(shape[0] == 2 * B for shape, _, _ in m.calls)          # one evaluation per step: the corrector costs none
    assert torch.equal(m.calls[0][2]['v'][:B], uc['v']) and torch.equal(m.calls[0][2]['v'][B:], c['v'])      # unconditional FIRST
    assert [t for _, t, _ in m.calls] == [int(t) for t in np.flip(sampler.Schedule().make_ddim(S).ddim_timesteps)]
    assert inter['x_inter'][0] is x_T and inter['x_inter'][-1] is out
    ts, a, ap = dref.grid(S)
    comb = uref.unipc(lambda x, t, cc: (0.1 * x - 1.0) + 3.0 * ((0.1 * x + 2.0) - (0.1 * x - 1.0)), ts, a, ap, x_T.double())
    torch.testing.assert_close(out.double(), comb, rtol=1e-5, atol=1e-5)
    m.calls.clear()
    UniPCSampler(m).sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T)
    assert len(m.calls) == S and all(shape[0] == B for shape, _, _ in m.calls)
    # the trace lists have DDIM's lengths, and the rescaled guidance is the torch form's
    from makeupdiffuse_amd.ddim import DDIMSampler
    for Lt in (1, 2, 3, 100):
        _, inter = UniPCSampler(m).sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, log_every_t=Lt)
        _, ddim = DDIMSampler(m).sample(S, B, (4, 3, 3), conditioning=c, x_T=x_T, log_every_t=Lt, eta=0.0, verbose=False)
        for key in ('x_inter', 'pred_x0'):
            assert len(inter[key]) == len(ddim[key]) == 1 + sample_log_rows(S, Lt), (key, Lt)
    g = torch.Generator().manual_seed(4)
    cw, uw = {'v': torch.randn(B, 4, 3, 3, generator=g)}, {'v': torch.randn(B, 4, 3, 3, generator=g)}
    plain, _ = UniPCSampler(m).sample(S, B, (4, 3, 3), conditioning=cw, x_T=x_T, unconditional_guidance_scale=3.0, unconditional_conditioning=uw)
    resc, _ = UniPCSampler(m).sample(S, B, (4, 3, 3), conditioning=cw, x_T=x_T, unconditional_guidance_scale=3.0, unconditional_conditioning=uw,
                                     guidance_rescale=0.7)
    assert (resc - plain).abs().max() > 1e-3


def test_fast_hook_gets_the_tables():
    m = HostModel(lambda x, t, c: 0.1 * x)
    S, B = 5, 2
    x_T = torch.randn(B, 4, 3, 3)
    seen = {}

    def fast(x, c, timesteps, alphas, alphas_prev, order, lower_order_final, corrector, scale=1.0, uc=None, **kw):
        seen.update(kw, timesteps=list(timesteps), alphas=list(alphas), alphas_prev=list(alphas_prev), order=order, lof=lower_order_final,
                    corrector=corrector, scale=scale, uc=uc)
        if 'log_every_t' in kw:
            r = sample_log_rows(len(timesteps), kw['log_every_t'])
            return x + 1.0, [x + float(j) for j in range(r)], [x - float(j) for j in range(r)]
        return x
    m.sample_loop_unipc = fast
    out, inter = UniPCSampler(m).sample(S, B, (4, 3, 3), x_T=x_T, order=3, lower_order_final=False, corrector=False, log_every_t=2)
    sch = sampler.Schedule().make_ddim(S)
    assert seen['timesteps'] == list(sch.ddim_timesteps) and seen['order'] == 3 and seen['lof'] is False and seen['corrector'] is False
    assert np.allclose(seen['alphas'], sch.ddim_alphas.numpy()) and np.allclose(seen['alphas_prev'], sch.ddim_alphas_prev.numpy())
    assert seen['log_every_t'] == 2 and 'guidance_rescale' not in seen and seen['scale'] == 1.0 and seen['uc'] is None
    assert not any(k in seen for k in ('x0', 'mask', 'q_noise'))
    rows = sample_log_rows(S, 2)
    assert len(inter['x_inter']) == len(inter['pred_x0']) == 1 + rows
    assert inter['x_inter'][0] is x_T and inter['x_inter'][-1] is out and torch.equal(out, x_T + 1.0)
    # guidance and its rescale reach the hook; without an unconditional half phi is not engaged
    uc = {'v': 1}
    UniPCSampler(m).sample(S, B, (4, 3, 3), x_T=x_T, unconditional_guidance_scale=4.0, unconditional_conditioning=uc, guidance_rescale=0.7)
    assert seen['scale'] == 4.0 and seen['uc'] is uc and seen['guidance_rescale'] == 0.7 and seen['corrector'] is True and seen['order'] == 2
    seen.clear()
    UniPCSampler(m).sample(S, B, (4, 3, 3), x_T=x_T, guidance_rescale=0.7)
    assert 'guidance_rescale' not in seen
    # a callback takes the per-step loop instead
    seen.clear()
    UniPCSampler(m).sample(S, B, (4, 3, 3), x_T=x_T, callback=lambda k: None)
    assert not seen


def test_decode_uses_the_first_t_start_entries():
    eps = lambda x, t, c: 0.2 * torch.tanh(x)
    m = HostModel(eps)
    s = UniPCSampler(m)
    s.make_schedule(10)
    x = torch.randn(1, 4, 3, 3, dtype=torch.float64)
    sch = sampler.Schedule().make_ddim(10)
    for t_start, order, cor in ((4, 2, True), (7, 3, True), (10, 2, False), (1, 2, True)):
        m.calls.clear()
        out = s.decode(x, None, t_start, order=order, corrector=cor)
        assert [t for _, t, _ in m.calls] == [int(t) for t in np.flip(sch.ddim_timesteps[:t_start])]
        ref = uref.unipc(eps, sch.ddim_timesteps[:t_start], sch.ddim_alphas[:t_start].numpy(), sch.ddim_alphas_prev[:t_start].numpy(),
                         x, order=order, corrector=cor)
        assert (out - ref).abs().max().item() <= 1e-12
    assert s.decode(x, None, 0) is x
    with pytest.raises(ValueError):
        s.decode(x, None, 11)
